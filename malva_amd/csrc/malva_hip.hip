// malva_hip.hip -- kernels and C ABI of the MI355X-native malva-geno hot path.
// See include/malva_hip.h for the interface and the reference lines each entry
// point replaces; DESIGN.md for the data layout and the roofline of each kernel.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h> // types and prototypes only: the library itself is opened on first use (mg_comm_*)

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "count_plan.h"
#include "gate_geometry.h"
#include "geno_dev.h"
#include "grm_plan.h"
#include "malva_hip.h"
#include "pca_plan.h"

using namespace mg;

#define MG_EXPORT extern "C" __attribute__((visibility("default")))

// ===========================================================================
// Kernels
// ===========================================================================

namespace {

constexpr size_t TK_META_HEAD = 8; // ticket meta block: spill count, then the segment fills
constexpr int BIN_SEGS = 2048; // workgroups of the binning kernel = segments per bin
constexpr int TPB = 256;
constexpr int GATE_RESIDENT_KIB = 3072;   // default of option gate_resident_kib (mg_ctx): swept 2048..4096 at C3, 3072 and 3584 tie on the whole step, 4096 loses 0.07 ms
constexpr int GATE_RESIDENT_MIN_BITS = 8; // a sized gate keeps at least this many bits per entry (8.4 at C3 with 2048 KiB still beat the 4 MiB gate, by 0.02 ms)

#include "store_kernels.h"
#include "scan_kernels.h"
#include "variant_kernels.h"
#include "block_pipeline.h"
#include "gt_text_kernels.h"
#include "call_text_kernels.h"
#include "site_tags_kernels.h"
#include "pair_kernels.h"
#include "sample_kernels.h"
#include "site_geno_kernels.h"
#include "ld_kernels.h"
#include "ibd_kernels.h"
#include "grm_kernels.h"
#include "pca_kernels.h"
#include "cohort_prior_kernels.h"
#include "bcf_kernels.h"
#include "pl_kernels.h"
#include "reads_kernels.h"

} // namespace

// ===========================================================================
// Host side: context, memory, launches
// ===========================================================================

struct BFState {
    u64 size = 0, nwords = 0, n_blk = 0, nset = 0;
    u64 *words = nullptr;
    u32 *blk = nullptr;
    u32 *counts = nullptr;
    u64 *gate = nullptr; // only `bf` (MG_BF_ALT) owns one
    u64 n_gate_bits = 0;
    u32 gate_shift = 6;
    u32 gate_words = 0, gate_mul = 0, gate_ls = 0, gate_rs = 0; // a gate sized in words (BFView::gate_words); 0: the shift form
    u64 *pos_set = nullptr; // `context_bf`, call time: its set positions as a hash set (BFView::pos_set); built at the first scan
    u32 pos_set_log2 = 0;
    bool pos_set_valid = false;
    u64 *pregate = nullptr; // coarse L2-sized gate in front of a gate that outgrew L2
    u32 pre_shift = 6;
    int mode = 0;
    ModDesc mod{};
};
struct MapState {
    u32 cap_log2 = 0;
    MapSlot *slots = nullptr; // `tags` in the comments below = the tag field of these records
    u32 *vals = nullptr;
    u64 rows_total = 0; // insertion rows so far (upper bound on distinct keys; ids index space)
    u64 vals_cap = 0;
    std::unordered_map<std::string, int32_t> irregular; // keys the packed table cannot hold (N / NUL-truncated)
};
struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
};
// One timed call of the record loop or of the merged-batch section: its events (the first n of them: start, then the end of each part) and
// whether they are those of a call that ran (timer_begin, timer_mark, timer_read).  TM_FMT .. TM_BCF are the three row encoders (encode_rows)
// and index s_enc too.
struct Timer {
    int n;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool valid = false;
};
enum { TM_FMT, TM_INFO, TM_BCF, TM_SITE, TM_PACK, TM_PAIR, TM_SAMPLE, TM_PRIOR, TM_ESTIMATE, TM_PL, TM_BLOCKS, TM_COHORT, TM_GENO, TM_HWE, TM_LD_PACK, TM_LD, TM_IBD_TR, TM_IBD, TM_COUNT }; // mg_format_calls*, mg_format_site_info*, mg_encode_calls_bcf*, mg_site_counts*, mg_pack_dosage*, mg_pair_counts*, mg_sample_counts*, mg_genotype_cohort*, mg_estimate_priors*, mg_phred_likelihoods*, mg_cover_blocks_device, mg_cover_blocks_cohort_device, mg_site_geno_counts*, mg_hwe_exact*, mg_pack_site_dosage*, mg_ld_window* (length pass, scan, write pass), mg_sites_to_planes*, mg_ibd_step*
enum { ENC_COUNT = TM_BCF + 1 };
// what an encoder's device form keeps from its length pass to its write pass: the rows' lengths (u32), the meta block (the total, "a row
// beyond 32 bits"), and (mg_encode_calls_bcf*) the records' type codes
enum { ES_LEN, ES_META, ES_TYPES, ES_COUNT };
// Device copies of the host forms' arguments and results, for every host form of the merged-batch section.  One set is enough: the caller
// serialises the host forms of a context, each runs on the context's stream and synchronises before it returns, so no staged buffer
// outlives its call; and no device form touches the set (those own s_enc and s_scan, and read and write the caller's buffers).
enum {
    ST_GT1, ST_GT2, ST_GQ, ST_COV, ST_VAR_ALLELE_OFF, ST_PROBS, ST_VAR_GT_OFF, ST_STATUS, ST_ALLELE_CLASS, // a batch's cells (stage_cells)
    ST_AC, ST_NS, ST_PLANES, ST_PA, ST_PB, ST_COUNTS,                                                      // the counting calls' tables
    ST_OUT, ST_ROW_OFF,                                                                                    // an encoder's rows (stage_rows)
    ST_FREQ, ST_FREQ_OUT, ST_NINF,                                                                         // mg_genotype_cohort's priors
    ST_PL,                                                                                                 // mg_phred_likelihoods' result, the *_pl encoders' input
    ST_SG_N, ST_SG_HET, ST_SG_HOM, ST_HWE, ST_EXC_HET,                                                     // mg_site_geno_counts' tables, mg_hwe_exact's items and results
    ST_LD_WORDS, ST_LD_SITES, ST_LD_CHROM, ST_LD_POS, ST_LD_PAIRS, ST_LD_ROW_OFF,                          // mg_pack_site_dosage's words; mg_ld_window's tables and pairs
    ST_IBD_SITES, ST_IBD_PLANES, ST_IBD_CHROM, ST_IBD_POS, ST_IBD_SEGS,                                    // mg_sites_to_planes' and mg_ibd_step's tables and segments
    ST_COUNT
};

struct mg_ctx {
    int device = 0;
    hipStream_t stream = nullptr, own_stream = nullptr;
    u32 k = 0, ref_k = 0;
    BFState bf[2];
    MapState map;
    Scratch s_rows, s_aux, s_out, s_irr, s_open[3], s_hit[4], s_misc[8], s_blk[16], s_gt[10], s_scan;
    void *h_gt_stage = nullptr;                       // pinned staging for mg_decode_gt_text's text (a pageable source is copied by the runtime in small synchronous pieces)
    size_t h_gt_stage_cap = 0;
    u32 gt_records = 0, gt_keep = 0, gt_default = 0; // the batch mg_decode_gt_text left on the device for mg_decode_gt_entries
    u64 gt_entries = 0;
    unsigned long long *d_gen_count = nullptr; // [0] records listed for cover_blocks_kernel, [1] insertion-row cursor / block count of a host-form batch,
                                               // [2] signature k-mers of the lone records, [3] of the others (mg_blocks_stats)
    int blocks_grid[3] = {0, 0, 0};            // persistent grid of cover_blocks_kernel<MODE> (found at first use)
    int use_flat_tier = 1;                     // 0: every general record takes the workgroup kernel (A/B, tests)
    // the records' own copies of their counters (MapSlot::cval / cbf): current for epoch rec_epoch while rec_ok.  Every ABI call
    // drops rec_ok on entry unless it is one of those that cannot change a counter behind the copies' back (DeviceGuard, KEEP).
    int use_record_counters = 1;
    mutable bool rec_ok = false;
    // lazy vectors: scans of the sub-slice form add to the records' copies alone while those are current (MapView::lazy); whoever
    // needs vals[] / counts[] afterwards -- an export, a per-k-mer call, an exchange, anything that ends the copies' validity --
    // first brings them up to date (vectors_current: one pass over the record table).  vec_zero: the vectors are known to be all
    // zero (mg_counters_reset then has nothing to clear: 0.7 GB per step at whole-genome scale)
    int lazy_vectors = 1;
    mutable bool vec_stale = false, vec_zero = false;
    bool rec_off = false;                      // the counter vector has been handed out (mg_counters_view): whoever holds it may write it
    u32 rec_epoch = 1;
    int blocks_round_log2 = 24;                // see blocks_setup
    int lone_tiles = 0;                        // record loop, tier 1: tiles a workgroup takes, 1 / 2 / 4 / 8; 0: by the panel's size (lone_tiles_for)
    int use_hit_entries = 1;                   // scan: the probe kernel hands the hit kernel each row's filter entry (counter index, record) with the row
    int use_snp_chains = 1;                    // record loop: chains of SNPs assembled as the reference window with the members' bases put in
    u64 last_rounds = 0;                       // rounds of tier 2 in the most recent record loop (blocks_listed_chains)
    int use_chain_kernel = 1;                  // record loop: the picks of a chain evaluated by the wave that holds them (fw_chain_kernel) instead of picks -> items -> eval
    int use_snp_kernel = 1;                    // record loop: chains of SNPs on panels of up to 8 diploid / 16 haploid samples in one kernel (fw_snp_kernel) instead of picks + eval
    int use_chain_order = 1;                   // record loop: what fw_snp_kernel left of a round's chains, listed in order of their number of members, before the
                                               // chain kernel takes them (fw_order_kernel: less divergence in the per-member loops, and no walk over descriptors
                                               // already dealt with)
    int use_packed_pool = 1;                   // record loop: signature k-mers assembled from 2-bit alleles (mg_panel_dev.pool_bytes) instead of bytes
    int map_ordered = 1;                       // records in order of the filter slot (map_home); fixed before the first key or filter entry goes in
    int map_dense = 0;                         // 1: record tables beyond 4 GB are sized at load 1/2 instead of 1/4 (measured at C4: the probe kernel got 25 % SLOWER -- longer walks, same translation cost)
    int use_ctx_set = 1;                       // 1: large context filters answer the scan's hit kernel from the set of their set positions (A/B)
    int use_packed_ref_scan = 1;               // 0: the byte-wise reference scan for every window (A/B, tests)
    unsigned long long *d_hit_count = nullptr;
    double *d_ln = nullptr;
    float *d_eps = nullptr; // [2 * MG_EPS_TABLE]
    float eps_for = -1.f;
    u8 *d_ref = nullptr;
    size_t ref_len = 0;
    u64 *d_ref2 = nullptr;   // the same reference as 2-bit codes (ref_pack_kernel) ...
    u32 *d_refbad = nullptr; // ... and one bit per base: not ACGT
    // scan timing (mg_scan_stats): four events per launch group (chunk) of the most recent scan, the first SCAN_EV_CHUNKS of them
    std::vector<hipEvent_t> ev;
    std::vector<u64> ev_rows; // rows of each timed chunk
    bool stats_valid = false;
    // cohort mode (mg_cohort_begin): bf[ALT].counts / map.vals hold coh_planes samples' counters side by side, sample-minor, a counter's
    // cells 2^coh_shift apart (the planes rounded up to a power of two); every view reads and writes plane coh_sel.  Counters live
    // in the vectors alone while it lasts (records_wanted), like a context in a group.  The single-sample vectors wait in coh_sv_*;
    // coh_irr: the host-side values of the keys the table cannot hold, per plane, and ([coh_planes]) the single-sample ones.
    u32 coh_planes = 0, coh_shift = 0, coh_sel = 0;
    u32 *coh_sv_counts = nullptr, *coh_sv_vals = nullptr;
    std::vector<std::unordered_map<std::string, int32_t>> coh_irr;
    // each stats call reports the latest call of its own kinds, hence a timer per kind: the encoders' four events, the counting calls' two;
    // mg_cover_blocks_device: before / after the preparation, the lone kernels, the enumerating kernel; mg_cover_blocks_cohort_device: start,
    // after tier 1, after the planes' tiers 2-3
    Timer tm[TM_COUNT] = {{4}, {4}, {4}, {2}, {2}, {2}, {2}, {2}, {2}, {2}, {4}, {3}, {2}, {2}, {2}, {4}, {2}, {2}};
    Scratch s_enc[ENC_COUNT][ES_COUNT], stage[ST_COUNT];
    // mg_ibd_begin .. mg_ibd_end: the pairs' state, five u32 arrays [n_pairs] and behind them the last record's chrom id (ibd_kernels.h);
    // s_ibd: a step's planes, start words, segment counts (u32), offsets (u64) and the meta block (the total)
    u32 *ibd_state = nullptr;
    u64 ibd_pairs = 0;
    u32 ibd_samples = 0, ibd_min_records = 0;
    long long ibd_min_bp = 0;
    Scratch s_ibd[5];
    // mg_grm_begin .. mg_grm_end: the pairs' state -- the sums (i64 [n_pairs]), the counts (u64 [n_pairs]) and behind them the number of
    // records that entered (u64) -- and the records seen (grm_kernels.h).  s_grm: a piece's weights and its three byte images; grm_in:
    // the host forms' words and weights.  grm_tm: start, behind weights + expand, behind gram, of the step's latest piece; grm_ms: the
    // pieces before it, and the latest read
    void *grm_state = nullptr;
    u64 grm_pairs = 0, grm_seen = 0;
    u32 grm_samples = 0, grm_maf_ppm = 0, grm_min_n = 0;
    int grm_haploid = 0;
    Scratch s_grm[2], grm_in[2];
    Timer grm_tm{3}, grm_read_tm{2};
    float grm_ms[3] = {0.f, 0.f, 0.f};
    bool grm_timed = false;
    int grm_scratch_mb = GRM_SCRATCH_MB; // the cap on a piece's byte images (tests: smaller, so that a step takes several pieces)
    // mg_pca_load* .. mg_pca_end: the resident matrix ([np][np] doubles, np = pca_np(n), and behind them the "a value is not finite" flag,
    // a u32), whether the flag has been read since the load, the blocks and small tables of a solve (pca_work), the host forms' input and
    // output (pca_io).  pca_ev: the events of a solve between two of its waits, pca_ev_phase[i] the phase the interval ending at event i
    // belongs to; pca_ms: products, orthonormalisation, Rayleigh-Ritz, total of the most recent solve.
    void *pca_g = nullptr;
    u32 pca_n = 0;
    bool pca_checked = false, pca_timed = false;
    Scratch pca_work, pca_io[2];
    std::vector<hipEvent_t> pca_ev;
    std::vector<int> pca_ev_phase;
    size_t pca_ev_used = 0;
    float pca_ms[4] = {0.f, 0.f, 0.f, 0.f};
    Scratch s_ld[2]; // mg_ld_window_device, from its length pass to its write pass: the records' pair counts (u32), the meta block (the total)
    u32 *joined = nullptr; // when set: one allocation holding [bf counters | map counters] (mg_counters_view)
    int use_summary = 1;
    bool gate_dirty = false; // something has been inserted into `bf`
    bool gate_fixed = false; // gate_log2 was set by the caller: do not resize at finalize
    int scan_rows = 2;    // table rows per thread per iteration of the filter kernel (swept: 2 is best)
    int scan_grid = 8192; // workgroups of the filter kernel (32 per CU; swept 2048..8192)
    int scan_ablate = 0;  // timing-only diagnostic, see scan_filter_kernel
    u32 iso_call_no = 0;  // mg_call_isolated calls so far (see iso_cover_kernel)
    u32 blocks_set_limit = BK_SET_CAP / 2; // cover_blocks_kernel: distinct picks per chain kept in LDS before it evaluates every pick
    int scan_variant = 2; // filter-kernel VAR bits (staging / load width): 16-byte loads measured best
    int pre_k = 1;      // bits per entry of the coarse gate (chosen at finalize from the load)
    int use_pregate = 1;
    bool pre_skip = false; // the coarse gate is saturated at this index size (decided at finalize): scans go straight to the fine gate
    int pregate_log2 = 25; // coarse gate size: 4 MiB, what stays resident in an XCD's L2 next to the table stream
    int use_partition = 0; // bin the coarse gate's survivors by fine-gate slice (SoA tables, fine gates of 4..64 MiB).  Off: since the ticket and sub-slice forms took the
                           // gates of 32 MiB and more, what is left to this form is where the plain filter kernel beats it (C5, 16 MiB gate: 0.84 against 1.03 ms per
                           // 1e8 rows; C3-shaped indexes of 4e6 and 8e6 entries: 0.82 / 1.09 against 0.96 / 1.23)
    int probe_grid = 2048, hits_grid = 1024; // workgroups of the two list kernels (swept)
    int use_tickets = 1;      // gates of 2^ticket_min_log2 bits and more: 8-byte tickets filed by 2 MiB gate slice, the slices then walked out of L2
                              // (scan_ticket_sort_kernel + scan_ticket_gate_kernel) instead of one random HBM sector per table row
    int tkg_grid = 0;         // pass two's grid: one workgroup per CU (found at first use)
    int chunk_log2 = 27;      // rows per launch group (tests shrink it to put many chunks into a small table)
    int ticket_min_log2 = 28; // smallest fine gate (log2 bits) that takes the ticket form: 32 MiB.  Measured on a C4 share (3.75e8 rows, compact rows):
                              // 16 MiB gate 3.6 ms two-level direct / 4.8 tickets; 32 MiB 7.7 / 6.2; 256 MiB 9.3 / 7.3 (profiles/r02_c4share_forms.txt)
    Scratch s_tk[2];
    unsigned long long *d_tk_meta = nullptr; // spill count, then u32 [TK_MAXP][BIN_SEGS] segment fills
    // the sub-slice form (scan_sub_sort_kernel + scan_sub_gate_kernel): tickets filed under LDS-sized pieces of the gate
    int use_sub = 1;          // gates of 2^sub_min_log2 bits and more (takes precedence over the ticket form; 0: A/B)
    int sub_min_log2 = 28;    // smallest fine gate (log2 bits) that takes it
    int sub_words_log2 = SB_WORDS_LOG2; // gate words per sub-slice (tests shrink it to put many bins into a small gate)
    int sub_bins_log2 = 10;   // the gate is sized (at finalize) to split into at most 2^sub_bins_log2 sub-slices (<= SB_MAXB).  Measured at one GPU's share of
                              // C4: 2,048 pieces (a 256 MiB gate, ~0.5 % false positives) leave pass one in runs of 8 tickets = 64 B and cost its stores and pass
                              // two 0.5 ms per 2^27 rows more than 1,024 pieces (128 MiB, ~4 %) cost the probe kernel (0.23 ms)
    int sub_split = 4;        // workgroups of the probe kernel per region of open rows
    int sub_grid = 0;         // pass one's grid (0: one workgroup per CU)
    int n_cus = 0;            // CUs of the device (found at first use)
    Scratch s_sb[4];          // tickets, spill list, open tickets, meta block (spill count, region counts, segment fills)
    int last_subs = 0;        // bins the most recent scan filed tickets under (0: it did not take this form)
    int bin_ring = 0, bin_rows = 4; // A/B: staging ring per bin (0 = as large as LDS allows), rows per thread of the binning kernel
    u64 bin_cap = 0;       // rows per bin segment; 0 = 1.5x an even share of the chunk (tests set it small to reach the spill path)
    int last_bins = 0;     // bins used by the most recent scan (0: direct form)
    int last_tickets = 0;  // gate slices the most recent scan filed tickets under (0: it did not)
    Scratch s_bin[3], s_spill[3];
    unsigned long long *d_bin_meta = nullptr; // spill count, then u32 [BIN_MAXP][BIN_SEGS] segment fills
    int gate_k = 4;     // gate bits per entry (blocked Bloom filter inside one 64-bit word; swept 2..4)
    int gate_log2 = 25; // gate of at most 2^gate_log2 bits (swept 24..26 among the powers of two: 25 = 4 MiB; such a gate is then allocated with gate_resident_kib, below)
    // A gate of exactly the L2 size leaves the table stream no room in L2 beside it: every stream line that allocates evicts a
    // gate line.  Where the sizing rule of mg_bf_finalize lands on 2^pregate_log2 = 2^25 bits and the direct single-level form scans, the gate is
    // allocated with gate_resident_kib KiB instead (no power of two: BFView::gate_words), unless that leaves an entry fewer than
    // GATE_RESIDENT_MIN_BITS bits.  0: keep the power of two.  (profiles/gate_span_sweep.txt)
    int gate_resident_kib = GATE_RESIDENT_KIB;
    u64 gate_words_opt = 0; // option gate_words (tests, A/B): the direct single-level form's gate has exactly this many words, whatever the index holds
    u64 gate_words = 0;     // words of the sized gate that alloc_gate makes (0: the shift form): set_option / mg_bf_finalize decide
    // multi-GPU exchange (mg_comm_*): an RCCL communicator, or -- contexts of one process that share a device, where
    // RCCL refuses duplicate ranks -- the list of contexts whose counters a kernel sums
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    std::vector<mg_ctx *> local_group;
    hipEvent_t ev_x = nullptr; // orders the local-group exchange between the contexts' streams
    // the exchange's own stream (mg_counters_allreduce_begin / _end: what needs no counters runs on the context's stream meanwhile),
    // its timing events, and the 16-bit packed form: two counters per word on the wire when no rank's partial counter can carry
    hipStream_t xstream = nullptr;
    hipEvent_t ev_xs[4] = {nullptr, nullptr, nullptr, nullptr}; // scan done / exchange done (ordering), exchange start / end (timing)
    bool x_pending = false, x_timed = false;
    int exchange_pack = 1;          // 0 never, 1 vectors of exchange_pack_min_mb and more, 2 always (when exact)
    int exchange_pack_min_mb = 32;
    int last_exchange_packed = 0;
    u32 *d_xmax = nullptr;
    Scratch s_pack;
    // host-fed scans (mg_kmc_scan, mg_kmc_scan_records): two staging slots, uploads on their own stream beside the scan
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_free[2] = {nullptr, nullptr};
    Scratch s_stage[2][3], s_raw[2];
    u64 *d_kmc_lut = nullptr; // <db>.kmc_pre's prefix table (+ guard), mg_kmc_set_lut
    u64 kmc_n_lut = 0;
    u32 kmc_prefix_len = 0, kmc_suffix_bytes = 0, kmc_counter_bytes = 0, kmc_min_count = 0;
    u64 kmc_max_count = 0;
    // counting from reads (mg_reads_*): the state of the current begin .. finish, and two tunables
    struct ReadsState *reads = nullptr;
    int reads_budget_mb = 4096; // pairs (20 B each) one pass may file
    int reads_passes = 0;       // at least this many passes (tests)
    int reads_parts_log2 = RD_PART_LOG2; // key partitions (tests: fewer, so that one bin outgrows LDS with distinct keys)
    std::string err;
};

namespace {

int fail(mg_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}
#define HIP_TRY(c, expr)                                                                                             \
    do {                                                                                                             \
        hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess)                                                                                        \
            return fail(c, e_ == hipErrorOutOfMemory ? MG_ERR_NOMEM : MG_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define TRY(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != MG_OK) return rc_; \
    } while (0)

inline unsigned nblocks(u64 n) { return (unsigned)((n + TPB - 1) / TPB); }
int comm_drop(mg_ctx *c); // multi-GPU section
void reads_drop(mg_ctx *c); // reads section
bool reads_unfinished(const mg_ctx *c); // reads section: between mg_reads_begin and mg_reads_finish

int scratch(mg_ctx *c, Scratch &s, size_t bytes, void **out)
{
    if (bytes > s.cap) {
        if (s.p) HIP_TRY(c, hipFree(s.p));
        s.p = nullptr;
        s.cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        HIP_TRY(c, hipMalloc(&s.p, want));
        s.cap = want;
    }
    *out = s.p;
    return MG_OK;
}
// exclusive scan of n_tiles u32 sums in place, their total (u64) to *d_total: store_kernels.h
int launch_tile_scan(mg_ctx *c, u32 *d_tiles, u64 n_tiles, unsigned long long *d_total)
{
    if (n_tiles <= SCAN_CHUNK) { // one workgroup's worth: one launch instead of three
        hipLaunchKernelGGL(tile_scan_small_kernel, dim3(1), dim3(SCAN_TPB), 0, c->stream, d_tiles, n_tiles, d_total);
        HIP_TRY(c, hipGetLastError());
        return MG_OK;
    }
    const u64 n_part = (n_tiles + SCAN_CHUNK - 1) / SCAN_CHUNK;
    void *part;
    TRY(scratch(c, c->s_scan, 8 * n_part, &part));
    hipLaunchKernelGGL(tile_reduce_kernel, dim3((unsigned)n_part), dim3(SCAN_TPB), 0, c->stream, (const u32 *)d_tiles, n_tiles, (unsigned long long *)part);
    hipLaunchKernelGGL(part_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, c->stream, (unsigned long long *)part, n_part, d_total);
    hipLaunchKernelGGL(tile_rescan_kernel, dim3((unsigned)n_part), dim3(SCAN_TPB), 0, c->stream, d_tiles, n_tiles, (const unsigned long long *)part);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int upload(mg_ctx *c, Scratch &s, const void *host, size_t bytes, void **dev)
{
    TRY(scratch(c, s, bytes ? bytes : 1, dev));
    if (bytes) HIP_TRY(c, hipMemcpyAsync(*dev, host, bytes, hipMemcpyHostToDevice, c->stream));
    return MG_OK;
}

// A call's timer: begin before its first work goes on the stream (an empty call counts as a call), mark(i) behind part i (the last mark
// makes the timer valid), read in the stats call: waits for the call, ms[i] = device milliseconds of part i + 1; 0 where no call has run
int timer_begin(mg_ctx *c, Timer &t)
{
    for (int i = 0; i < t.n; ++i)
        if (!t.ev[i]) HIP_TRY(c, hipEventCreate(&t.ev[i]));
    t.valid = false;
    HIP_TRY(c, hipEventRecord(t.ev[0], c->stream));
    return MG_OK;
}
int timer_mark(mg_ctx *c, Timer &t, int i)
{
    HIP_TRY(c, hipEventRecord(t.ev[i], c->stream));
    if (i == t.n - 1) t.valid = true;
    return MG_OK;
}
int timer_read(mg_ctx *c, const Timer &t, float *ms)
{
    if (t.valid) HIP_TRY(c, hipEventSynchronize(t.ev[t.n - 1]));
    for (int i = 0; i + 1 < t.n; ++i) {
        ms[i] = 0.f;
        if (t.valid) HIP_TRY(c, hipEventElapsedTime(&ms[i], t.ev[i], t.ev[i + 1]));
    }
    return MG_OK;
}

ModDesc make_mod(u64 size)
{
    ModDesc m{};
    m.size = size;
    u32 sh = 0;
    u64 odd = size;
    while (odd && !(odd & 1)) {
        odd >>= 1;
        ++sh;
    }
    m.shift = sh;
    m.odd = odd;
    if (odd == 1) m.kind = 0;
    else if (odd < (1ULL << 32) && sh >= 32) m.kind = 1;
    else m.kind = 2;
    return m;
}

// use_pregate: 0 never, 1 unless saturated (pre_skip), 2 always (tests)
bool pregate_on(const mg_ctx *c) { return c->use_pregate == 2 || (c->use_pregate == 1 && !c->pre_skip); }

BFView view(const mg_ctx *c, int which)
{
    const BFState &b = c->bf[which];
    BFView v{};
    v.words = b.words;
    v.blk = b.blk;
    v.counts = b.counts;
    v.gate = b.gate;
    v.mod = b.mod;
    v.gate_shift = b.gate_shift;
    v.gate_k = (u32)c->gate_k;
    v.gate_words = b.gate_words;
    v.gate_mul = b.gate_mul;
    v.gate_ls = b.gate_ls;
    v.gate_rs = b.gate_rs;
    v.pregate = pregate_on(c) ? b.pregate : nullptr;
    v.pregate_fill = b.pregate; // filled whenever it exists, so use_pregate / pre_skip may change between scans
    v.pre_shift = b.pre_shift;
    v.pre_k = (u32)c->pre_k;
    v.use_gate = (c->use_summary && b.gate) ? 1 : 0;
    v.pos_set = b.pos_set_valid ? b.pos_set : nullptr;
    v.pos_set_log2 = b.pos_set_log2;
    if (which == MG_BF_ALT) v.cshift = c->coh_shift, v.coff = c->coh_sel; // (0 and 0 outside cohort mode)
    return v;
}
// Are the records' counter copies worth keeping?  They cost the scan a compare-and-swap per hit beside its add to the vector
// and save a lookup its second random line.  While vals[] / counts[] stay in the caches (C3: 8 MB) that line is cheap and
// the copies lose (measured: 1.043 against 1.000 ms per C3 step); beyond that they win (use_record_counters: 0 never, 2 always).
bool records_wanted(const mg_ctx *c)
{
    if (!c->use_record_counters || c->rec_off || c->comm_world > 1 || !c->local_group.empty() || c->coh_planes) return false;
    return c->use_record_counters >= 2 || (u64)(c->bf[MG_BF_ALT].nset + c->map.rows_total) * 4 > (256ull << 20);
}
MapView view(const mg_ctx *c)
{
    const MapState &m = c->map;
    MapView v{};
    v.slots = m.slots;
    v.vals = m.vals;
    v.cshift = c->coh_shift;
    v.coff = c->coh_sel;
    v.cap_log2 = m.cap_log2;
    v.klen = c->k;
    v.home_mul = c->map_ordered ? ~0ULL / c->bf[MG_BF_ALT].mod.size : 0x9E3779B97F4A7C15ULL;
    v.epoch = c->rec_ok && records_wanted(c) ? c->rec_epoch : 0;
    v.lazy = v.epoch && c->lazy_vectors ? 1u : 0u;
    return v;
}

// give the two counter arrays their own allocations again (before either has to be resized)
int unjoin(mg_ctx *c)
{
    if (!c->joined) return MG_OK;
    BFState &b = c->bf[MG_BF_ALT];
    MapState &m = c->map;
    u32 *nc = nullptr, *nv = nullptr;
    HIP_TRY(c, hipMalloc(&nc, (b.nset ? b.nset : 1) * 4));
    HIP_TRY(c, hipMalloc(&nv, (m.vals_cap ? m.vals_cap : 1) * 4));
    if (b.nset) HIP_TRY(c, hipMemcpyAsync(nc, b.counts, b.nset * 4, hipMemcpyDeviceToDevice, c->stream));
    if (m.vals_cap) HIP_TRY(c, hipMemcpyAsync(nv, m.vals, m.vals_cap * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipFree(c->joined);
    c->joined = nullptr;
    b.counts = nc;
    m.vals = nv;
    return MG_OK;
}

// (the geometry of a gate sized in words: gate_geometry.h)
u64 gate_words_max(const BFState &b) { return std::min<u64>(std::max<u64>(1, b.size / 64), 1ULL << 30); }
// Words of the sized gate that takes the place of a gate of 2^want bits over `entries` entries; 0: the power of two stays.  Only
// where the direct single-level form scans (no coarse gate; the ticket and sub-slice forms cut the gate by word index) and the
// caller did not fix the size.
u64 sized_gate_words(const mg_ctx *c, int want, u64 entries)
{
    if (c->gate_fixed || want > c->pregate_log2) return 0;
    if (c->use_sub && want >= c->sub_min_log2) return 0;
    if (c->use_tickets && want >= c->ticket_min_log2) return 0;
    if (c->gate_words_opt) return c->gate_words_opt;
    const u64 bits = (u64)c->gate_resident_kib * 8192; // (want == pregate_log2: the gate is exactly what the context takes for an XCD's L2)
    if (want != c->pregate_log2 || !bits || bits >= (1ULL << want) || bits < (u64)GATE_RESIDENT_MIN_BITS * entries) return 0;
    return bits / 64;
}

// (re)allocate the gate of `bf`: at most 2^gate_log2 bits, one per 2^gate_shift filter bits -- or, for a gate sized in words
// (mg_ctx::gate_words != 0), that many words
int alloc_gate(mg_ctx *c)
{
    BFState &b = c->bf[MG_BF_ALT];
    u32 S = 6;
    while (((b.size + (1ULL << S) - 1) >> S) > (1ULL << c->gate_log2)) ++S;
    b.gate_shift = S;
    b.n_gate_bits = (b.size + (1ULL << S) - 1) >> S;
    b.gate_words = b.gate_mul = b.gate_ls = b.gate_rs = 0;
    if (c->gate_words && c->gate_log2 <= c->pregate_log2) { // (no coarse gate in front of a sized one)
        b.gate_words = (u32)std::min<u64>(c->gate_words, gate_words_max(b));
        gate_geometry(b.size, b.gate_words, &b.gate_mul, &b.gate_ls, &b.gate_rs, &b.gate_shift);
        b.n_gate_bits = 64ULL * b.gate_words;
    }
    if (b.gate) HIP_TRY(c, hipFree(b.gate));
    b.gate = nullptr;
    const size_t bytes = ((b.n_gate_bits + 63) / 64) * 8;
    HIP_TRY(c, hipMalloc(&b.gate, bytes));
    HIP_TRY(c, hipMemsetAsync(b.gate, 0, bytes, c->stream));
    if (b.pregate) HIP_TRY(c, hipFree(b.pregate));
    b.pregate = nullptr;
    if (c->gate_log2 > c->pregate_log2) { // the gate no longer fits L2: coarse gate of the L2-resident size in front of it
        u32 S1 = 6;
        while (((b.size + (1ULL << S1) - 1) >> S1) > (1ULL << c->pregate_log2)) ++S1;
        b.pre_shift = S1;
        const size_t pbytes = ((((b.size + (1ULL << S1) - 1) >> S1) + 63) / 64) * 8;
        HIP_TRY(c, hipMalloc(&b.pregate, pbytes));
        HIP_TRY(c, hipMemsetAsync(b.pregate, 0, pbytes, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

int map_alloc(mg_ctx *c, MapState &m, u32 cap_log2)
{
    const u64 cap = 1ULL << cap_log2;
    m.cap_log2 = cap_log2;
    HIP_TRY(c, hipMalloc(&m.slots, cap * sizeof(MapSlot)));
    hipLaunchKernelGGL(map_clear_kernel, dim3(nblocks(cap)), dim3(TPB), 0, c->stream, m.slots, cap);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
void map_free_table(MapState &m)
{
    hipFree(m.slots);
    m.slots = nullptr;
}
// (re)write the filter's directory into the records: whenever the finalised filter's bits or the table change
int build_bf_entries(mg_ctx *c)
{
    const BFState &alt = c->bf[MG_BF_ALT];
    MapState &m = c->map;
    if (!m.slots || !alt.mode || !alt.blk) return MG_OK;
    const u64 cap = 1ULL << m.cap_log2;
    hipLaunchKernelGGL(bf_entries_clear_kernel, dim3(nblocks(cap)), dim3(TPB), 0, c->stream, m.slots, cap);
    hipLaunchKernelGGL(bf_entries_build_kernel, dim3(nblocks(alt.nwords)), dim3(TPB), 0, c->stream, view(c, MG_BF_ALT), view(c), alt.nwords);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}

// make room for `extra` more insertion rows: table load <= 1/4, vals indexable by row
int map_reserve(mg_ctx *c, u64 extra)
{
    MapState &m = c->map;
    const u64 need_rows = m.rows_total + extra;
    if (c->coh_planes && extra) return fail(c, MG_ERR_STATE, "the index is fixed while the context is in cohort mode (mg_cohort_end first)");
    if (need_rows >= 0xFFFFFFFFULL) return fail(c, MG_ERR_LIMIT, "exact map: more than 2^32-1 insertion rows");
    if (need_rows > m.vals_cap) {
        TRY(unjoin(c));
        u64 ncap = need_rows + need_rows / 2 + 1024;
        u32 *nv = nullptr;
        HIP_TRY(c, hipMalloc(&nv, ncap * 4));
        HIP_TRY(c, hipMemsetAsync(nv, 0, ncap * 4, c->stream));
        if (m.vals && m.rows_total)
            HIP_TRY(c, hipMemcpyAsync(nv, m.vals, m.rows_total * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (m.vals) hipFree(m.vals);
        m.vals = nv;
        m.vals_cap = ncap;
    }
    // records: load <= 1/4 for the keys, and two filter-directory entries per record at load <= 1/4 as well
    const BFState &alt = c->bf[MG_BF_ALT];
    const u64 dir_entries = alt.mode ? alt.nset : 0;
    u32 want = 10;
    while ((1ULL << want) < need_rows * 4 || (1ULL << want) < dir_entries * 2) ++want;
    if (want > 26 && c->map_dense) {
        // Beyond 2^26 records (4 GB) what a probe costs is the PAGE it lands on, not the length of its walk: at whole-genome scale
        // scan_probe_kernel spent its time in address translation (UTCL2 busy 93 %, profiles/r03_pmc_c4share_before.txt), and the next
        // record of a walk is nearly always on the same page.  Half the table: key load <= 1/2, directory load <= 1/2.
        u32 w2 = 26;
        while ((1ULL << w2) < need_rows * 2 || (1ULL << w2) < dir_entries) ++w2;
        if (w2 < want) want = w2;
    }
    if (!m.slots) {
        TRY(map_alloc(c, m, want));
        return build_bf_entries(c);
    }
    if (want > m.cap_log2) {
        MapView ov{};
        ov.slots = m.slots;
        ov.cap_log2 = m.cap_log2;
        ov.klen = c->k;
        ov.home_mul = view(c).home_mul;
        m.slots = nullptr;
        TRY(map_alloc(c, m, want));
        MapView nv = view(c);
        hipLaunchKernelGGL(map_rehash_kernel, dim3(nblocks(1ULL << ov.cap_log2)), dim3(TPB), 0, c->stream, ov, nv, c->bf[MG_BF_ALT].mod);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        hipFree(ov.slots);
        return build_bf_entries(c); // the new records start without the filter's directory
    }
    return MG_OK;
}

int check_rows(mg_ctx *c, const void *rows, size_t stride, size_t n)
{
    if (!c) return MG_ERR_ARG;
    if (n && !rows) return fail(c, MG_ERR_ARG, "rows is NULL");
    if (stride < 2) return fail(c, MG_ERR_ARG, "row stride %zu too small", stride);
    return MG_OK;
}
int check_which(mg_ctx *c, int which)
{
    if (!c) return MG_ERR_ARG;
    if (which != MG_BF_ALT && which != MG_BF_CTX) return fail(c, MG_ERR_ARG, "which must be MG_BF_ALT or MG_BF_CTX");
    return MG_OK;
}

template <int OP>
int run_rows(mg_ctx *c, int which, const char *rows, size_t stride, size_t n, const void *counters, const u8 *is_ref,
             void *host_out, size_t out_elem, u8 *host_irregular)
{
    if (n == 0) return MG_OK;
    void *d_rows, *d_cnt = nullptr, *d_isref = nullptr, *d_out = nullptr, *d_irr = nullptr;
    TRY(upload(c, c->s_rows, rows, stride * n, &d_rows));
    if (counters) TRY(upload(c, c->s_aux, counters, 4 * n, &d_cnt));
    if (is_ref) TRY(upload(c, c->s_misc[0], is_ref, n, &d_isref));
    if (host_out) TRY(scratch(c, c->s_out, out_elem * n, &d_out));
    if (host_irregular) TRY(scratch(c, c->s_irr, n, &d_irr));
    hipLaunchKernelGGL(rows_kernel<OP>, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const u8 *)d_rows, stride, n,
                       view(c, which), view(c), (const u32 *)d_cnt, (const u8 *)d_isref, d_out, (u8 *)d_irr);
    HIP_TRY(c, hipGetLastError());
    if (host_out) HIP_TRY(c, hipMemcpyAsync(host_out, d_out, out_elem * n, hipMemcpyDeviceToHost, c->stream));
    if (host_irregular) HIP_TRY(c, hipMemcpyAsync(host_irregular, d_irr, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// canonical key of an irregular row as KMAP::canonical returns it (kmap.hpp:86-97):
// bookkeeping for keys the device table cannot represent; the scan never sees them.
std::string host_irregular_key(const char *row, size_t stride)
{
    size_t k = strnlen(row, stride);
    std::string rc(k, '\0');
    auto comp = [](unsigned char ch) -> char {
        switch (ch) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; case 'N': return 'N';
        case 'a': return 'T'; case 'c': return 'G'; case 'g': return 'G'; case 't': return 'A'; case 'n': return 'N';
        default: return 0;
        }
    };
    for (size_t i = 0; i < k; ++i) rc[i] = comp((unsigned char)row[k - 1 - i]);
    std::string fw(row, k);
    bool fwd = false;
    for (size_t i = 0; i < k; ++i)
        if ((unsigned char)fw[i] != (unsigned char)rc[i]) {
            fwd = (unsigned char)fw[i] < (unsigned char)rc[i];
            break;
        }
    std::string can = fwd ? fw : rc;
    return std::string(can.c_str()); // cut at the first NUL
}

int fill_geno_params(mg_ctx *c, float error_rate, int max_cov, int haploid, GenoParams *p)
{
    if (!c->d_ln) {
        std::vector<double> t(MG_LN_TABLE);
        t[0] = 0.0;
        for (int n = 1; n < MG_LN_TABLE; ++n) t[n] = std::log((double)n);
        HIP_TRY(c, hipMalloc(&c->d_ln, sizeof(double) * MG_LN_TABLE));
        HIP_TRY(c, hipMemcpy(c->d_ln, t.data(), sizeof(double) * MG_LN_TABLE, hipMemcpyHostToDevice));
    }
    if (!c->d_eps) HIP_TRY(c, hipMalloc(&c->d_eps, sizeof(float) * 2 * MG_EPS_TABLE));
    if (!(c->eps_for == error_rate)) {
        std::vector<float> t(2 * MG_EPS_TABLE, 0.f);
        for (int A = 0; A < MG_EPS_TABLE; ++A) {
            t[A] = std::log(error_rate / (float)(unsigned long)(A - 1));                // float overload
            t[MG_EPS_TABLE + A] = std::log(error_rate / (float)(unsigned long)(A - 2)); // float overload
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_eps, t.data(), sizeof(float) * 2 * MG_EPS_TABLE, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->eps_for = error_rate;
    }
    p->ln_tab = c->d_ln;
    p->c_err1 = c->d_eps;
    p->c_err2 = c->d_eps + MG_EPS_TABLE;
    p->c_hom = std::log(1 - error_rate);
    p->c_het = std::log((1 - error_rate) / 2);
    p->error_rate = error_rate;
    p->max_cov = max_cov;
    p->haploid = haploid;
    return MG_OK;
}

// genotype_one (geno_dev.h) on the host, every log and exp from libm: for the records of mg_genotype whose total coverage
// is at or beyond MG_LN_TABLE, where the kernel's ln(n) is the device's log(double) and about one value in a thousand
// comes out a last bit away from the CPU path.  The operations of gt_value and of the general form of
// genotype_one in their order; the biallelic form of the kernel is the same sequence unrolled.
double host_log_binomial(int n, int k)
{
    if (n == 0 || n == k || k == 0) return 0.0;
    const double a = n * std::log((double)n);
    const double b = k * std::log((double)k);
    const double c = (n - k) * std::log((double)(n - k));
    return a - b - c;
}
double host_gt_value(const u32 *cov, const float *freq, int A, u32 total, int g1, int g2, float e)
{
    double log_prior, log_post;
    if (g2 < 0 || g1 == g2) {
        const u32 truth = cov[g1], error = total - truth;
        log_prior = (double)(2 * std::log(freq[g1])); // float overload, here and below
        const float t1 = (float)truth * std::log(1 - e);
        const float t2 = (float)error * std::log(e / (float)(unsigned long)(A - 1));
        log_post = host_log_binomial((int)(truth + error), (int)truth) + (double)t1 + (double)t2;
    } else {
        const u32 t1c = cov[g1], t2c = cov[g2], error = total - t1c - t2c;
        const float pr = 2 * freq[g1] * freq[g2];
        log_prior = (double)std::log(pr);
        const float c_het = std::log((1 - e) / 2);
        const float t1 = (float)t1c * c_het;
        const float t2 = (float)t2c * c_het;
        log_post = host_log_binomial((int)(t1c + t2c + error), (int)(t1c + t2c)) + host_log_binomial((int)(t1c + t2c), (int)t1c) + (double)t1 + (double)t2;
        if (A > 2) {
            const float t3 = (float)error * std::log(e / (float)(unsigned long)(A - 2));
            log_post += (double)t3;
        }
    }
    const double lp = log_prior + log_post;
    return std::isinf(lp) ? 0.0 : std::exp(lp);
}
// one record of status 0: gt1 / gt2 / gq and, if probs != nullptr, the normalised list
void host_genotype_one(const u32 *cov, const float *freq, int A, u32 total, float e, int haploid, i32 *gt1, i32 *gt2, i32 *gq, double *probs)
{
    std::vector<double> val;
    val.reserve(haploid ? (size_t)A : (size_t)A * (A + 1) / 2);
    std::vector<int> a1, a2;
    double sum = 0.0;
    for (int g1 = 0; g1 < A; ++g1)
        for (int g2 = haploid ? -1 : g1; g2 < (haploid ? 0 : A); ++g2) {
            val.push_back(host_gt_value(cov, freq, A, total, g1, g2, e));
            a1.push_back(g1);
            a2.push_back(g2);
            sum += val.back();
        }
    double best = 0.0;
    *gt1 = 0;
    *gt2 = haploid ? -1 : 0;
    for (size_t n = 0; n < val.size(); ++n) {
        const double q = val[n] / sum;
        if (probs) probs[n] = q;
        if (q > best) {
            best = q;
            *gt1 = a1[n];
            *gt2 = a2[n];
        }
    }
    *gq = (i32)std::round(best * 100.0);
}

} // namespace

// ---- lifetime -------------------------------------------------------------------

// Every entry point may be called from any host thread: make the context's device current for the calling thread
// (HIP's current device is per thread; a thread that never called hipSetDevice sits on device 0).
// for DeviceGuard.  KEEP: this entry point leaves the counters alone, or changes them together with the records' copies (it may READ the
// vectors: they are brought up to date first).  LAZY: the same, and it never looks at vals[] / counts[] while the copies are current
// (the scans, the record loop's device forms, the bookkeeping calls): lazy vectors stay lazy.
constexpr int KEEP = 1, LAZY = 2;
// vals[] / counts[] from the records' copies, where scans have added to the copies alone
void vectors_current(const mg_ctx *c)
{
    if (!c->vec_stale) return;
    c->vec_stale = false;
    c->vec_zero = false;
    if (!c->map.slots || !c->rec_ok) return; // (cannot happen: lazy scans need current copies, and nothing drops them without coming through here)
    MapView m = view(c);
    m.epoch = c->rec_epoch;
    hipLaunchKernelGGL(rec_collect_kernel, dim3((unsigned)std::min<u64>(nblocks(1ULL << m.cap_log2), 1u << 20)), dim3(TPB), 0, c->stream, m,
                       c->bf[MG_BF_ALT].mode ? c->bf[MG_BF_ALT].counts : (u32 *)nullptr, c->rec_epoch);
}
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(const mg_ctx *c, int keeps_record_counters = 0)
    {
        int cur = -1;
        if (c && hipGetDevice(&cur) == hipSuccess && cur != c->device && hipSetDevice(c->device) == hipSuccess) prev = cur;
        if (c && keeps_record_counters != LAZY) vectors_current(c);
        if (c && !keeps_record_counters) c->rec_ok = false, c->vec_zero = false;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) hipSetDevice(prev); // leave the caller's thread as it was
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

MG_EXPORT int mg_create(mg_ctx **out, int device, uint32_t k, uint32_t ref_k, uint64_t bf_bits)
{
    if (!out) return MG_ERR_ARG;
    *out = nullptr;
    if (k == 0 || k > MG_MAX_KMER || ref_k < k || ref_k > MG_MAX_KMER || bf_bits == 0) return MG_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return MG_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return MG_ERR_HIP;
    mg_ctx *c = new mg_ctx();
    c->device = device;
    c->k = k;
    c->ref_k = ref_k;
    if (hipStreamCreate(&c->own_stream) != hipSuccess) {
        delete c;
        return MG_ERR_HIP;
    }
    c->stream = c->own_stream;
    for (auto &e : c->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            delete c;
            return MG_ERR_HIP;
        }
    for (int w = 0; w < 2; ++w) {
        BFState &b = c->bf[w];
        b.size = bf_bits;
        b.nwords = (bf_bits + 63) / 64;
        b.n_blk = (b.nwords + 7) / 8;
        b.mod = make_mod(bf_bits);
        // whole 512-bit blocks (zero padded): lookups read the block of a bit in one go
        if (hipMalloc(&b.words, b.n_blk * 64) != hipSuccess || hipMemsetAsync(b.words, 0, b.n_blk * 64, c->stream) != hipSuccess) {
            mg_destroy(c);
            return MG_ERR_NOMEM;
        }
    }
    if (alloc_gate(c) != MG_OK || hipMalloc(&c->d_hit_count, 40) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
        mg_destroy(c);
        return MG_ERR_HIP;
    }
    *out = c;
    return MG_OK;
}

MG_EXPORT int mg_destroy(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (!c) return MG_OK;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    comm_drop(c);
    reads_drop(c);
    if (c->ev_x) hipEventDestroy(c->ev_x);
    for (auto &e : c->ev_xs)
        if (e) hipEventDestroy(e);
    if (c->xstream) hipStreamDestroy(c->xstream);
    hipFree(c->d_xmax);
    hipFree(c->s_pack.p);
    for (int i = 0; i < 2; ++i) {
        if (c->ev_up[i]) hipEventDestroy(c->ev_up[i]);
        if (c->ev_free[i]) hipEventDestroy(c->ev_free[i]);
        for (auto &q : c->s_stage[i]) hipFree(q.p);
        hipFree(c->s_raw[i].p);
    }
    if (c->copy_stream) hipStreamDestroy(c->copy_stream);
    if (c->h_gt_stage) hipHostFree(c->h_gt_stage);
    hipFree(c->d_kmc_lut);
    hipFree(c->coh_sv_counts);
    hipFree(c->coh_sv_vals);
    for (Timer &t : c->tm)
        for (hipEvent_t e : t.ev)
            if (e) hipEventDestroy(e);
    for (auto &enc : c->s_enc)
        for (Scratch &q : enc) hipFree(q.p);
    for (Scratch &q : c->stage) hipFree(q.p);
    for (Scratch &q : c->s_ld) hipFree(q.p);
    for (Scratch &q : c->s_ibd) hipFree(q.p);
    hipFree(c->ibd_state);
    for (Scratch &q : c->s_grm) hipFree(q.p);
    for (Scratch &q : c->grm_in) hipFree(q.p);
    hipFree(c->grm_state);
    hipFree(c->pca_g);
    hipFree(c->pca_work.p);
    for (Scratch &q : c->pca_io) hipFree(q.p);
    for (hipEvent_t e : c->pca_ev) hipEventDestroy(e);
    for (Timer *t : {&c->grm_tm, &c->grm_read_tm})
        for (hipEvent_t e : t->ev)
            if (e) hipEventDestroy(e);
    if (c->joined) { // the two counter arrays alias one allocation
        hipFree(c->joined);
        c->bf[MG_BF_ALT].counts = nullptr;
        c->map.vals = nullptr;
    }
    for (auto &b : c->bf) {
        hipFree(b.words);
        hipFree(b.blk);
        hipFree(b.counts);
        hipFree(b.gate);
        hipFree(b.pregate);
        hipFree(b.pos_set);
    }
    map_free_table(c->map);
    hipFree(c->map.vals);
    for (Scratch *s : {&c->s_rows, &c->s_aux, &c->s_out, &c->s_irr}) hipFree(s->p);
    for (auto &s : c->s_open) hipFree(s.p);
    for (auto &s : c->s_bin) hipFree(s.p);
    for (auto &s : c->s_spill) hipFree(s.p);
    hipFree(c->d_bin_meta);
    hipFree(c->d_tk_meta);
    for (auto &q : c->s_tk) hipFree(q.p);
    for (auto &q : c->s_sb) hipFree(q.p);
    for (auto &s : c->s_hit) hipFree(s.p);
    for (auto &s : c->s_misc) hipFree(s.p);
    for (auto &s : c->s_blk) hipFree(s.p);
    for (auto &s : c->s_gt) hipFree(s.p);
    hipFree(c->s_scan.p);
    hipFree(c->d_gen_count);
    hipFree(c->d_hit_count);
    hipFree(c->d_ln);
    hipFree(c->d_eps);
    hipFree(c->d_ref);
    hipFree(c->d_ref2);
    hipFree(c->d_refbad);
    for (auto &e : c->ev)
        if (e) hipEventDestroy(e);
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
    return MG_OK;
}

MG_EXPORT const char *mg_last_error(const mg_ctx *c) { return c ? c->err.c_str() : "null context"; }

MG_EXPORT int mg_set_stream(mg_ctx *c, void *s)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return MG_OK;
}
MG_EXPORT int mg_synchronize(mg_ctx *c)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}
MG_EXPORT int mg_set_option(mg_ctx *c, const char *name, int64_t value)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || !name) return MG_ERR_ARG;
    if (!strcmp(name, "use_summary")) c->use_summary = value != 0;
    else if (!strcmp(name, "scan_rows")) c->scan_rows = (int)value;
    else if (!strcmp(name, "scan_ablate")) c->scan_ablate = (int)value;
    else if (!strcmp(name, "blocks_set_limit")) c->blocks_set_limit = (u32)std::min<int64_t>(std::max<int64_t>(value, 0), BK_SET_CAP / 2);
    else if (!strcmp(name, "use_pregate")) c->use_pregate = value < 0 ? 0 : value > 2 ? 2 : (int)value;
    else if (!strcmp(name, "use_partition")) c->use_partition = value != 0;
    else if (!strcmp(name, "use_flat_tier")) c->use_flat_tier = value != 0;
    else if (!strcmp(name, "map_dense")) c->map_dense = value != 0;
    else if (!strcmp(name, "use_packed_pool")) c->use_packed_pool = value != 0;
    else if (!strcmp(name, "use_snp_chains")) c->use_snp_chains = value != 0;
    else if (!strcmp(name, "use_hit_entries")) c->use_hit_entries = value != 0;
    else if (!strcmp(name, "blocks_round_log2")) {
        if (value < 10 || value > 24) return fail(c, MG_ERR_ARG, "blocks_round_log2: 10..24");
        c->blocks_round_log2 = (int)value;
    }
    else if (!strcmp(name, "lone_tiles")) {
        if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8) return fail(c, MG_ERR_ARG, "lone_tiles: 0 (by the panel's size), 1, 2, 4 or 8");
        c->lone_tiles = (int)value;
    }
    else if (!strcmp(name, "map_ordered")) {
        if (c->map.slots && (value != 0) != (c->map_ordered != 0)) return fail(c, MG_ERR_STATE, "map_ordered is a layout: set it before the index is built or loaded");
        c->map_ordered = value != 0;
    }
    else if (!strcmp(name, "use_record_counters")) {
        c->use_record_counters = value < 0 ? 0 : value > 2 ? 2 : (int)value;
        c->rec_ok = false; // (the next scan brings the copies up to date)
    }
    else if (!strcmp(name, "use_ctx_set")) {
        c->use_ctx_set = (int)value; // (2: whatever the filter's size -- tests)
        c->bf[MG_BF_CTX].pos_set_valid = false;
    }
    else if (!strcmp(name, "use_packed_ref_scan")) c->use_packed_ref_scan = value != 0;
    else if (!strcmp(name, "probe_grid")) c->probe_grid = value > 0 ? (int)value : 2048;
    else if (!strcmp(name, "use_tickets")) c->use_tickets = value != 0;
    else if (!strcmp(name, "use_sub")) c->use_sub = value != 0;
    else if (!strcmp(name, "use_chain_order")) c->use_chain_order = value != 0;
    else if (!strcmp(name, "use_chain_kernel")) c->use_chain_kernel = value != 0;
    else if (!strcmp(name, "use_snp_kernel")) c->use_snp_kernel = value != 0;
    else if (!strcmp(name, "exchange_pack")) c->exchange_pack = (int)std::max<int64_t>(0, std::min<int64_t>(2, value));
    else if (!strcmp(name, "exchange_pack_min_mb")) c->exchange_pack_min_mb = (int)std::max<int64_t>(0, value);
    else if (!strcmp(name, "lazy_vectors")) c->lazy_vectors = value != 0;
    else if (!strcmp(name, "sub_min_log2")) c->sub_min_log2 = (int)value;
    else if (!strcmp(name, "sub_words_log2")) {
        if (value < 0 || value > SB_WORDS_LOG2) return fail(c, MG_ERR_ARG, "sub_words_log2 must be 0..%d", SB_WORDS_LOG2);
        c->sub_words_log2 = (int)value;
    } else if (!strcmp(name, "sub_bins_log2")) c->sub_bins_log2 = (int)std::max<int64_t>(1, std::min<int64_t>(10, value));
    else if (!strcmp(name, "sub_split")) c->sub_split = (int)std::max<int64_t>(1, std::min<int64_t>(64, value));
    else if (!strcmp(name, "sub_grid")) c->sub_grid = (int)std::max<int64_t>(0, std::min<int64_t>(SB_MAXB, value)); // (nseg <= SB_MAXB: a wave of scan_sub_gate_kernel keeps its segments' fills one per lane)
    else if (!strcmp(name, "ticket_min_log2")) c->ticket_min_log2 = (int)value;
    else if (!strcmp(name, "scan_chunk_log2")) c->chunk_log2 = (int)std::min<int64_t>(27, std::max<int64_t>(10, value));
    else if (!strcmp(name, "ticket_gate_grid")) c->tkg_grid = value > 0 ? (int)std::max<int64_t>(8, std::min<int64_t>(4096, value / 8 * 8)) : 0;
    else if (!strcmp(name, "hits_grid")) c->hits_grid = value > 0 ? (int)value : 1024;
    else if (!strcmp(name, "scan_bin_cap")) c->bin_cap = value > 0 ? (u64)value : 0;
    else if (!strcmp(name, "scan_bin_ring")) {
        if (value != 0 && value != 64 && value != 128 && value != 256) return fail(c, MG_ERR_ARG, "scan_bin_ring must be 0, 64, 128 or 256");
        c->bin_ring = (int)value;
    }
    else if (!strcmp(name, "scan_bin_rows")) c->bin_rows = value == 2 ? 2 : 4;
    else if (!strcmp(name, "pregate_log2")) {
        if (c->map.rows_total || c->gate_dirty) return fail(c, MG_ERR_STATE, "pregate_log2 must be set before the first insert");
        if (value < 8 || value > 30) return fail(c, MG_ERR_ARG, "pregate_log2 must be 8..30");
        c->pregate_log2 = (int)value;
        return alloc_gate(c);
    }
    else if (!strcmp(name, "reads_budget_mb")) c->reads_budget_mb = (int)std::max<int64_t>(1, std::min<int64_t>(1 << 20, value));
    else if (!strcmp(name, "reads_passes")) c->reads_passes = (int)std::max<int64_t>(0, std::min<int64_t>(RD_PARTS, value));
    else if (!strcmp(name, "reads_parts_log2")) c->reads_parts_log2 = (int)std::max<int64_t>(0, std::min<int64_t>(RD_PART_LOG2, value));
    else if (!strcmp(name, "grm_scratch_mb")) c->grm_scratch_mb = (int)std::max<int64_t>(1, std::min<int64_t>(4096, value));
    else if (!strcmp(name, "scan_variant")) c->scan_variant = (int)value & 2;
    else if (!strcmp(name, "scan_grid")) c->scan_grid = value > 0 ? (int)value : 8192;
    else if (!strcmp(name, "gate_log2") || !strcmp(name, "gate_k") || !strcmp(name, "gate_words") || !strcmp(name, "gate_resident_kib")) {
        if (c->map.rows_total || c->gate_dirty) return fail(c, MG_ERR_STATE, "%s must be set before the first insert", name);
        if (!strcmp(name, "gate_k")) {
            if (value < 1 || value > 4) return fail(c, MG_ERR_ARG, "gate_k must be 1..4");
            c->gate_k = (int)value;
        } else if (!strcmp(name, "gate_resident_kib")) { // (takes effect when mg_bf_finalize sizes the gate)
            if (value < 0 || value > 4096) return fail(c, MG_ERR_ARG, "gate_resident_kib must be 0..4096");
            c->gate_resident_kib = (int)value;
            return MG_OK;
        } else if (!strcmp(name, "gate_words")) { // 0: back to the sizing rule
            if (value < 0 || value > (1LL << 30)) return fail(c, MG_ERR_ARG, "gate_words must be 0..2^30");
            c->gate_words_opt = (u64)value;
            c->gate_words = value ? sized_gate_words(c, c->gate_log2, 0) : 0;
        } else {
            c->gate_log2 = (int)value;
            c->gate_fixed = true;
            c->gate_words = 0;
        }
        return alloc_gate(c);
    }
    else return fail(c, MG_ERR_ARG, "unknown option %s", name);
    return MG_OK;
}

MG_EXPORT int mg_get_option(mg_ctx *c, const char *name, int64_t *value)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !name || !value) return MG_ERR_ARG;
    if (!strcmp(name, "use_summary")) *value = c->use_summary;
    else if (!strcmp(name, "use_pregate")) *value = c->use_pregate;
    else if (!strcmp(name, "use_partition")) *value = c->use_partition;
    else if (!strcmp(name, "use_flat_tier")) *value = c->use_flat_tier;
    else if (!strcmp(name, "map_dense")) *value = c->map_dense;
    else if (!strcmp(name, "use_packed_pool")) *value = c->use_packed_pool;
    else if (!strcmp(name, "use_snp_chains")) *value = c->use_snp_chains;
    else if (!strcmp(name, "use_hit_entries")) *value = c->use_hit_entries;
    else if (!strcmp(name, "use_chain_order")) *value = c->use_chain_order;
    else if (!strcmp(name, "blocks_listed_chains")) { // diagnostic: chains fw_chain_kernel handed to the list path in the most recent record loop (waits for it)
        unsigned long long total = 0;
        if (c->last_rounds && c->s_blk[5].p) {
            std::vector<unsigned long long> h((size_t)FW_ROUND_COUNTERS * c->last_rounds);
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipMemcpy(h.data(), c->s_blk[5].p, 8 * h.size(), hipMemcpyDeviceToHost));
            for (u64 r = 0; r < c->last_rounds; ++r) total += h[(size_t)FW_ROUND_COUNTERS * r + 3];
        }
        *value = (int64_t)total;
    }
    else if (!strcmp(name, "use_chain_kernel")) *value = c->use_chain_kernel;
    else if (!strcmp(name, "use_snp_kernel")) *value = c->use_snp_kernel;
    else if (!strcmp(name, "blocks_round_log2")) *value = c->blocks_round_log2;
    else if (!strcmp(name, "lone_tiles")) *value = c->lone_tiles;
    else if (!strcmp(name, "map_ordered")) *value = c->map_ordered;
    else if (!strcmp(name, "use_record_counters")) *value = c->use_record_counters;
    else if (!strcmp(name, "record_counters_live")) *value = view(c).epoch != 0; // diagnostic: would a lookup launched now read the records' copies?
    else if (!strcmp(name, "use_ctx_set")) *value = c->use_ctx_set;
    else if (!strcmp(name, "ctx_set_log2")) *value = c->bf[MG_BF_CTX].pos_set_valid ? c->bf[MG_BF_CTX].pos_set_log2 : 0;
    else if (!strcmp(name, "use_packed_ref_scan")) *value = c->use_packed_ref_scan;
    else if (!strcmp(name, "gate_log2")) *value = c->gate_log2;
    else if (!strcmp(name, "gate_k")) *value = c->gate_k;
    else if (!strcmp(name, "gate_words")) *value = c->bf[MG_BF_ALT].gate_words; // words of a gate sized in words; 0: a power-of-two gate of at most 2^gate_log2 bits
    else if (!strcmp(name, "gate_resident_kib")) *value = c->gate_resident_kib;
    else if (!strcmp(name, "pregate_log2")) *value = c->pregate_log2;
    else if (!strcmp(name, "pregate_k")) *value = c->bf[MG_BF_ALT].pregate && pregate_on(c) ? c->pre_k : 0;
    else if (!strcmp(name, "scan_bins")) *value = c->last_bins;
    else if (!strcmp(name, "scan_tickets")) *value = c->last_tickets;
    else if (!strcmp(name, "scan_subs")) *value = c->last_subs;
    else if (!strcmp(name, "use_sub")) *value = c->use_sub;
    else if (!strcmp(name, "sub_grid")) *value = c->sub_grid;
    else if (!strcmp(name, "exchange_pack")) *value = c->exchange_pack;
    else if (!strcmp(name, "exchange_packed")) *value = c->last_exchange_packed;
    else if (!strcmp(name, "lazy_vectors")) *value = c->lazy_vectors;
    else if (!strcmp(name, "vectors_stale")) *value = c->vec_stale;
    else if (!strcmp(name, "ticket_gate_grid")) *value = c->tkg_grid;
    else if (!strcmp(name, "use_tickets")) *value = c->use_tickets;
    else if (!strcmp(name, "reads_budget_mb")) *value = c->reads_budget_mb;
    else if (!strcmp(name, "reads_passes")) *value = c->reads_passes;
    else if (!strcmp(name, "reads_parts_log2")) *value = c->reads_parts_log2;
    else if (!strcmp(name, "grm_scratch_mb")) *value = c->grm_scratch_mb;
    else if (!strcmp(name, "scan_spilled")) { // rows of the last chunk that took the spill list
        unsigned long long t = 0;
        if (c->last_bins || c->last_tickets || c->last_subs) {
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipMemcpy(&t, c->last_subs ? c->s_sb[3].p : c->last_tickets ? (void *)c->d_tk_meta : (void *)c->d_bin_meta, 8, hipMemcpyDeviceToHost));
        }
        *value = (int64_t)t;
    }
    else return fail(c, MG_ERR_ARG, "unknown option %s", name);
    return MG_OK;
}

// ---- BF ---------------------------------------------------------------------------

MG_EXPORT int mg_bf_insert(mg_ctx *c, int which, const char *rows, size_t stride, size_t n)
{
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (c && (which == MG_BF_ALT || which == MG_BF_CTX)) c->bf[which].pos_set_valid = false; // (the bits are about to change)
    const DeviceGuard on_device(c);
    TRY(check_which(c, which));
    TRY(check_rows(c, rows, stride, n));
    // the reference lets add_key run in read mode too (the bit is set, the rank goes stale); refuse that
    if (c->bf[which].mode) return fail(c, MG_ERR_STATE, "mg_bf_insert after mg_bf_finalize");
    if (which == MG_BF_ALT) c->gate_dirty = true;
    return run_rows<OP_BF_INSERT>(c, which, rows, stride, n, nullptr, nullptr, nullptr, 0, nullptr);
}
MG_EXPORT int mg_bf_test(mg_ctx *c, int which, const char *rows, size_t stride, size_t n, uint8_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    TRY(check_rows(c, rows, stride, n));
    if (n && !out) return fail(c, MG_ERR_ARG, "out is NULL");
    return run_rows<OP_BF_TEST>(c, which, rows, stride, n, nullptr, nullptr, out, 1, nullptr);
}
MG_EXPORT int mg_debug_bf_index(mg_ctx *c, int which, const char *rows, size_t stride, size_t n, uint64_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    TRY(check_rows(c, rows, stride, n));
    if (n && !out) return fail(c, MG_ERR_ARG, "out is NULL");
    return run_rows<OP_BF_INDEX>(c, which, rows, stride, n, nullptr, nullptr, out, 8, nullptr);
}

MG_EXPORT int mg_bf_finalize(mg_ctx *c, int which)
{
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (c && (which == MG_BF_ALT || which == MG_BF_CTX)) c->bf[which].pos_set_valid = false;
    const DeviceGuard on_device(c);
    TRY(check_which(c, which));
    BFState &b = c->bf[which];
    if (b.blk) {
        hipFree(b.blk);
        b.blk = nullptr;
    }
    HIP_TRY(c, hipMalloc(&b.blk, (b.n_blk + 1) * 4));
    const u64 n_tiles = nblocks(b.n_blk + 1);
    void *d_tiles;
    TRY(scratch(c, c->s_misc[1], (n_tiles + 1) * 4, &d_tiles));
    unsigned long long *d_total = c->d_hit_count;
    hipLaunchKernelGGL(blk_pop_kernel, dim3((unsigned)n_tiles), dim3(TPB), 0, c->stream, b.words, b.nwords, b.n_blk, b.blk,
                       (u32 *)d_tiles);
    TRY(launch_tile_scan(c, (u32 *)d_tiles, n_tiles, d_total));
    HIP_TRY(c, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (total >= 0xFFFFFFFFULL) return fail(c, MG_ERR_LIMIT, "filter holds %llu set bits (>= 2^32-1)", total);
    hipLaunchKernelGGL(blk_add_kernel, dim3((unsigned)n_tiles), dim3(TPB), 0, c->stream, b.blk, b.n_blk, (const u32 *)d_tiles,
                       (u32)total);
    HIP_TRY(c, hipGetLastError());
    if (which == MG_BF_ALT) TRY(unjoin(c));
    b.nset = total;
    if (b.counts) hipFree(b.counts);
    b.counts = nullptr;
    HIP_TRY(c, hipMalloc(&b.counts, (total ? total : 1) * 4));
    HIP_TRY(c, hipMemsetAsync(b.counts, 0, (total ? total : 1) * 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b.mode = 1;
    if (which == MG_BF_ALT && !c->gate_fixed) {
        // size the gate for what the index holds: >= 12 bits per entry (set bf bits + exact-map keys), a power
        // of two, never below the default.  2e6 entries (C3) -> 2^25 bits = 4 MiB; 2e7 -> 2^28 = 32 MiB.
        const u64 entries = b.nset + c->map.rows_total;
        int want = 25;
        while (want < 34 && (1ULL << want) < 12 * entries) ++want;
        while (want > 6 && (1ULL << want) > b.size) --want;
        // an index that takes the sub-slice form (tickets filed under LDS-sized pieces of the gate) keeps its gate within
        // 2^sub_bins_log2 <= SB_MAXB pieces: 256 MiB at full-size pieces
        if (c->use_summary && c->use_sub && want >= c->sub_min_log2) want = std::min(want, c->sub_words_log2 + 6 + c->sub_bins_log2);
        // coarse gate: the bits per entry that minimise its false-positive rate at this load (ln 2 * bits / entries)
        int pk = entries ? (int)std::lround(0.6931 * (double)(1ULL << c->pregate_log2) / (double)entries) : 4;
        pk = pk < 1 ? 1 : pk > 4 ? 4 : pk;
        // a coarse gate that would let more than 3 of 4 rows through costs an L2 probe per row and saves little
        c->pre_skip = std::pow(1.0 - std::exp(-(double)pk * (double)entries / (double)(1ULL << c->pregate_log2)), pk) > 0.75;
        // a gate of exactly the L2 size gives way to one that stays resident beside the table stream (mg_ctx::gate_resident_kib)
        const u64 words = sized_gate_words(c, want, entries);
        if (want != c->gate_log2 || words != c->gate_words || (want > c->pregate_log2 && pk != c->pre_k)) {
            c->gate_log2 = want;
            c->gate_words = words;
            c->pre_k = pk;
            TRY(alloc_gate(c));
            hipLaunchKernelGGL(gate_from_bits_kernel, dim3(nblocks(b.nwords)), dim3(TPB), 0, c->stream, view(c, MG_BF_ALT), b.nwords);
            if (c->map.slots)
                hipLaunchKernelGGL(map_gate_kernel, dim3(nblocks(1ULL << c->map.cap_log2)), dim3(TPB), 0, c->stream, view(c),
                                   view(c, MG_BF_ALT));
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    if (which == MG_BF_ALT) { // the filter's directory inside the exact map's records (MapSlot)
        const bool had = c->map.slots != nullptr;
        const u32 before = c->map.cap_log2;
        TRY(map_reserve(c, 0)); // creates or grows the table if the directory needs it, and then writes the directory
        if (had && c->map.cap_log2 == before) TRY(build_bf_entries(c));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return MG_OK;
}

MG_EXPORT int mg_bf_increment(mg_ctx *c, int which, const char *rows, size_t stride, size_t n, const uint32_t *counters)
{
    const DeviceGuard on_device(c);
    TRY(check_which(c, which));
    TRY(check_rows(c, rows, stride, n));
    if (!c->bf[which].mode) return fail(c, MG_ERR_STATE, "BF::increment in write mode returns false");
    if (n && !counters) return fail(c, MG_ERR_ARG, "counters is NULL");
    return run_rows<OP_BF_INC>(c, which, rows, stride, n, counters, nullptr, nullptr, 0, nullptr);
}
MG_EXPORT int mg_bf_get_count(mg_ctx *c, int which, const char *rows, size_t stride, size_t n, uint16_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    TRY(check_rows(c, rows, stride, n));
    if (n && !out) return fail(c, MG_ERR_ARG, "out is NULL");
    if (!c->bf[which].mode) { // bloom_filter.hpp:117: write mode -> 0
        memset(out, 0, 2 * n);
        return MG_OK;
    }
    return run_rows<OP_BF_GET>(c, which, rows, stride, n, nullptr, nullptr, out, 2, nullptr);
}
MG_EXPORT int mg_bf_info(mg_ctx *c, int which, uint64_t *size_bits, uint64_t *n_set, int *mode)
{
    const DeviceGuard on_device(c, LAZY);
    TRY(check_which(c, which));
    if (size_bits) *size_bits = c->bf[which].size;
    if (n_set) *n_set = c->bf[which].nset;
    if (mode) *mode = c->bf[which].mode;
    return MG_OK;
}

// ---- KMAP ---------------------------------------------------------------------------

MG_EXPORT int mg_map_insert(mg_ctx *c, const char *rows, size_t stride, size_t n)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    TRY(check_rows(c, rows, stride, n));
    if (n == 0) return MG_OK;
    TRY(map_reserve(c, n));
    void *d_rows, *d_irr;
    TRY(upload(c, c->s_rows, rows, stride * n, &d_rows));
    TRY(scratch(c, c->s_irr, n, &d_irr));
    hipLaunchKernelGGL(map_insert_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const u8 *)d_rows, stride, n, view(c),
                       view(c, MG_BF_ALT), (u32)c->map.rows_total, (u8 *)d_irr);
    HIP_TRY(c, hipGetLastError());
    std::vector<u8> irr(n);
    HIP_TRY(c, hipMemcpyAsync(irr.data(), d_irr, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->map.rows_total += n;
    for (size_t i = 0; i < n; ++i)
        if (irr[i]) c->map.irregular[host_irregular_key(rows + i * stride, stride)] = 0;
    return MG_OK;
}
MG_EXPORT int mg_map_test(mg_ctx *c, const char *rows, size_t stride, size_t n, uint8_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_rows(c, rows, stride, n));
    if (n == 0) return MG_OK;
    if (!out) return fail(c, MG_ERR_ARG, "out is NULL");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    std::vector<u8> irr(n);
    TRY(run_rows<OP_MAP_TEST>(c, 0, rows, stride, n, nullptr, nullptr, out, 1, irr.data()));
    for (size_t i = 0; i < n; ++i)
        if (irr[i]) out[i] = c->map.irregular.count(host_irregular_key(rows + i * stride, stride)) ? 1 : 0;
    return MG_OK;
}
MG_EXPORT int mg_map_increment(mg_ctx *c, const char *rows, size_t stride, size_t n, const int32_t *counters)
{
    const DeviceGuard on_device(c);
    TRY(check_rows(c, rows, stride, n));
    if (n == 0) return MG_OK;
    if (!counters) return fail(c, MG_ERR_ARG, "counters is NULL");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    std::vector<u8> irr(n);
    TRY(run_rows<OP_MAP_INC>(c, 0, rows, stride, n, counters, nullptr, nullptr, 0, irr.data()));
    for (size_t i = 0; i < n; ++i)
        if (irr[i]) {
            auto it = c->map.irregular.find(host_irregular_key(rows + i * stride, stride));
            if (it != c->map.irregular.end()) it->second = (int32_t)((uint32_t)it->second + (uint32_t)counters[i]);
        }
    return MG_OK;
}
MG_EXPORT int mg_map_get_count(mg_ctx *c, const char *rows, size_t stride, size_t n, int32_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_rows(c, rows, stride, n));
    if (n == 0) return MG_OK;
    if (!out) return fail(c, MG_ERR_ARG, "out is NULL");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    std::vector<u8> irr(n);
    TRY(run_rows<OP_MAP_GET>(c, 0, rows, stride, n, nullptr, nullptr, out, 4, irr.data()));
    for (size_t i = 0; i < n; ++i)
        if (irr[i]) {
            auto it = c->map.irregular.find(host_irregular_key(rows + i * stride, stride));
            out[i] = it != c->map.irregular.end() ? it->second : 0;
        }
    return MG_OK;
}

namespace {
// distinct regular keys on the device table
int map_dump(mg_ctx *c, std::vector<u64> *klo, std::vector<u64> *khi, std::vector<u32> *ids)
{
    MapState &m = c->map;
    klo->clear();
    khi->clear();
    ids->clear();
    if (!m.slots) return MG_OK;
    const u64 cap = 1ULL << m.cap_log2;
    const u64 maxn = m.rows_total < cap ? m.rows_total : cap;
    if (maxn == 0) return MG_OK;
    void *d_lo, *d_hi, *d_id;
    TRY(scratch(c, c->s_misc[2], maxn * 8, &d_lo));
    TRY(scratch(c, c->s_misc[3], maxn * 8, &d_hi));
    TRY(scratch(c, c->s_misc[4], maxn * 4, &d_id));
    unsigned long long *d_n = c->d_hit_count + 4; // (a word of its own, not word 0: an export after a scan leaves the open-row count mg_scan_stats reports alone.  mg_bf_finalize and the record loop still reuse the scan's words)
    HIP_TRY(c, hipMemsetAsync(d_n, 0, 8, c->stream));
    hipLaunchKernelGGL(map_dump_kernel, dim3(nblocks(cap)), dim3(TPB), 0, c->stream, view(c), (u64 *)d_lo, (u64 *)d_hi,
                       (u32 *)d_id, d_n);
    HIP_TRY(c, hipGetLastError());
    unsigned long long cnt = 0;
    HIP_TRY(c, hipMemcpyAsync(&cnt, d_n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    klo->resize(cnt);
    khi->resize(cnt);
    ids->resize(cnt);
    if (cnt) {
        HIP_TRY(c, hipMemcpy(klo->data(), d_lo, cnt * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(khi->data(), d_hi, cnt * 8, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(ids->data(), d_id, cnt * 4, hipMemcpyDeviceToHost));
    }
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_map_size(mg_ctx *c, uint64_t *n_keys)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !n_keys) return MG_ERR_ARG;
    std::vector<u64> a, b;
    std::vector<u32> ids;
    TRY(map_dump(c, &a, &b, &ids));
    *n_keys = a.size() + c->map.irregular.size();
    return MG_OK;
}

// ---- reference scan --------------------------------------------------------------------

namespace {
int reference_pack(mg_ctx *c, const u8 *d_ascii, size_t len, u64 *ref2, u32 *refbad)
{
    const u64 n_words = (len + 31) / 32 + 4; // (+ the padding the span readers may touch)
    hipLaunchKernelGGL(ref_pack_kernel, dim3(nblocks(n_words)), dim3(TPB), 0, c->stream, d_ascii, (u64)len, ref2, refbad, n_words);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
// the windows [w0, w0 + nw) of a contig whose ASCII bytes from window w0 on are at d_ascii and whose base w0 sits at `at` in
// the packed arrays: the packed kernel, then the byte-wise one for what it leaves out
int ref_scan_windows(mg_ctx *c, const u8 *d_ascii, const u64 *ref2, const u32 *refbad, u64 at, u64 w0, u64 nw)
{
    const bool packed = c->k >= 1 && c->ref_k <= MG_MAX_PACKED_K && c->use_packed_ref_scan;
    if (packed) {
        const unsigned grid = (unsigned)std::min<u64>(nblocks((nw + REF_SCAN_W - 1) / REF_SCAN_W), 1u << 16);
        // (window numbers are contig-wide only through w == 0 and w < k: the packed kernel is handed the slice's own numbering
        //  shifted by w0 through `at` -- see its `w` -- so slices after the first never meet the quirk)
        if (c->k == 35 && c->ref_k == 43)
            hipLaunchKernelGGL((ref_scan_packed_kernel<35, 43>), dim3(grid), dim3(TPB), 0, c->stream, ref2, refbad, at, w0, nw, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c, MG_BF_CTX));
        else if (c->k == 35 && c->ref_k == 63)
            hipLaunchKernelGGL((ref_scan_packed_kernel<35, 63>), dim3(grid), dim3(TPB), 0, c->stream, ref2, refbad, at, w0, nw, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c, MG_BF_CTX));
        else
            hipLaunchKernelGGL((ref_scan_packed_kernel<0, 0>), dim3(grid), dim3(TPB), 0, c->stream, ref2, refbad, at, w0, nw, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c, MG_BF_CTX));
    }
    hipLaunchKernelGGL(ref_scan_kernel, dim3(nblocks(nw)), dim3(TPB), 0, c->stream, d_ascii, w0, nw, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c, MG_BF_CTX),
                       packed ? refbad : (const u32 *)nullptr, at);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int ref_scan_checks(mg_ctx *c, size_t len)
{
    c->bf[MG_BF_CTX].pos_set_valid = false;
    if (!c->bf[MG_BF_ALT].mode) return fail(c, MG_ERR_STATE, "mg_ref_scan needs `bf` finalised (main.cpp:378 precedes :383)");
    if (c->bf[MG_BF_CTX].mode) return fail(c, MG_ERR_STATE, "context filter already finalised");
    const size_t off = (c->ref_k - c->k) / 2;
    if (off > len) return fail(c, MG_ERR_ARG, "contig shorter than (ref_k-k)/2: the reference throws std::out_of_range here");
    return MG_OK;
}
// main.cpp:386-389 for a contig shorter than ref_k, both strings clipped by std::string(reference, pos, n): one test, no loop
int ref_scan_short(mg_ctx *c, const char *contig, size_t len)
{
    const size_t off = (c->ref_k - c->k) / 2;
    const size_t kn = len - off < c->k ? len - off : c->k;
    if (kn == 0) return fail(c, MG_ERR_ARG, "contig of %zu bases has no centre k-mer", len);
    std::vector<char> r1(MG_MAX_KMER + 8, 0), r2(MG_MAX_KMER + 8, 0);
    memcpy(r1.data(), contig + off, kn);
    memcpy(r2.data(), contig, len);
    uint8_t hit = 0;
    TRY(mg_bf_test(c, MG_BF_ALT, r1.data(), r1.size(), 1, &hit));
    if (hit) TRY(mg_bf_insert(c, MG_BF_CTX, r2.data(), r2.size(), 1));
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_ref_scan(mg_ctx *c, const char *contig, size_t len)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (len && !contig) return fail(c, MG_ERR_ARG, "contig is NULL");
    TRY(ref_scan_checks(c, len));
    if (len < c->ref_k) return ref_scan_short(c, contig, len);
    const u64 n_windows = len - c->ref_k + 1;
    // stream the contig through the device in slices (a human chromosome is a few hundred MB): bytes up, packed, scanned
    const size_t slice = 256u << 20;
    for (u64 w0 = 0; w0 < n_windows; w0 += slice) {
        const u64 nw = n_windows - w0 < slice ? n_windows - w0 : slice;
        const size_t nbytes = nw + c->ref_k - 1;
        void *d, *p2, *pb;
        TRY(scratch(c, c->s_rows, (nbytes + 63) / 64 * 64 + 256, &d));
        TRY(scratch(c, c->s_aux, ((nbytes + 31) / 32 + 4) * 8, &p2));
        TRY(scratch(c, c->s_out, ((nbytes + 31) / 32 + 4) * 4, &pb));
        HIP_TRY(c, hipMemsetAsync((u8 *)d + nbytes / 64 * 64, 0, (nbytes + 63) / 64 * 64 + 256 - nbytes / 64 * 64, c->stream)); // (the tail the pack kernel reads past the bytes)
        HIP_TRY(c, hipMemcpyAsync(d, contig + w0, nbytes, hipMemcpyHostToDevice, c->stream));
        TRY(reference_pack(c, (const u8 *)d, nbytes, (u64 *)p2, (u32 *)pb));
        TRY(ref_scan_windows(c, (const u8 *)d, (const u64 *)p2, (const u32 *)pb, 0, w0, nw));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the scratch is reused by the next slice; the caller may reuse its buffer)
    }
    return MG_OK;
}

// the same for a contig that lies at [offset, offset + len) of the buffer given to mg_reference_upload: nothing crosses PCIe
MG_EXPORT int mg_ref_scan_resident(mg_ctx *c, uint64_t offset, size_t len)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (!c->d_ref) return fail(c, MG_ERR_STATE, "mg_reference_upload first");
    if (offset + len > c->ref_len) return fail(c, MG_ERR_ARG, "contig lies outside the uploaded reference");
    TRY(ref_scan_checks(c, len));
    if (len < c->ref_k) { // (the short-contig case goes through the row kernels: fetch its bytes)
        std::vector<char> h(len + 1, 0);
        if (len) HIP_TRY(c, hipMemcpy(h.data(), c->d_ref + offset, len, hipMemcpyDeviceToHost));
        return ref_scan_short(c, h.data(), len);
    }
    const u64 n_windows = len - c->ref_k + 1;
    TRY(ref_scan_windows(c, c->d_ref + offset, c->d_ref2, c->d_refbad, offset, 0, n_windows));
    return MG_OK;
}

// ---- KMC scan ----------------------------------------------------------------------------

namespace {
// `context_bf` for the hit kernel: its set positions as a hash set, (re)built at the first scan after the bits changed
// Before a scan: bring the records' counter copies up to date (one pass over the record table, once after anything
// other than a scan has changed a counter: an index load, an import, a per-k-mer increment).  A context that is part of
// a multi-GPU group, or whose counter vector has been handed out, keeps its counters in the vectors alone.
int records_current(mg_ctx *c)
{
    if (!records_wanted(c)) {
        vectors_current(c);
        c->rec_ok = false;
        return MG_OK;
    }
    if (c->rec_ok || !c->map.slots) return MG_OK;
    if (++c->rec_epoch == 0) c->rec_epoch = 1; // (0 means "no copies"; the pass below rewrites every record that holds anything, so no older epoch survives it)
    MapView m = view(c);
    hipLaunchKernelGGL(rec_publish_kernel, dim3((unsigned)std::min<u64>(nblocks(1ULL << m.cap_log2), 1u << 20)), dim3(TPB), 0, c->stream, m,
                       (const u32 *)(c->bf[MG_BF_ALT].mode ? c->bf[MG_BF_ALT].counts : nullptr), c->rec_epoch);
    HIP_TRY(c, hipGetLastError());
    c->rec_ok = true;
    return MG_OK;
}
int ctx_set_ready(mg_ctx *c)
{
    BFState &b = c->bf[MG_BF_CTX];
    if (b.pos_set_valid) return MG_OK;
    // worth it where the bit array is far larger than the set: filters of 2^31 bits and more (256 MB) holding few bits
    u32 log2 = 10;
    while ((1ULL << log2) < 2 * b.nset + 16) ++log2;
    const bool want = c->use_ctx_set == 2 || (c->use_ctx_set == 1 && b.size >= (1ULL << 31) && (8ULL << log2) * 4 <= b.size / 8);
    if (!want) return MG_OK;
    if (b.pos_set) hipFree(b.pos_set);
    b.pos_set = nullptr;
    HIP_TRY(c, hipMalloc(&b.pos_set, 8ULL << log2));
    HIP_TRY(c, hipMemsetAsync(b.pos_set, 0, 8ULL << log2, c->stream));
    hipLaunchKernelGGL(pos_set_build_kernel, dim3(nblocks(b.nwords)), dim3(TPB), 0, c->stream, (const u64 *)b.words, b.nwords, b.pos_set, log2);
    HIP_TRY(c, hipGetLastError());
    b.pos_set_log2 = log2;
    b.pos_set_valid = true;
    return MG_OK;
}
// ---- the ticket form's host side ---------------------------------------------------------------------------------------
u64 ticket_slices(mg_ctx *c) // slices of half the L2-resident size (2 MiB) the fine gate splits into
{
    const u32 word_shift = (u32)(c->pregate_log2 - 1 - 6);
    return (((c->bf[MG_BF_ALT].n_gate_bits + 63) / 64) + (1ULL << word_shift) - 1) >> word_shift;
}
// segments, staging and meta block for launch groups of up to `cap` rows
int ticket_layout(mg_ctx *c, u64 cap, u32 row_bits, TicketSet *out)
{
    TicketSet tks{};
    const u64 TP = ticket_slices(c);
    tks.nbins = (u32)TP;
    tks.word_shift = (u32)(c->pregate_log2 - 1 - 6);
    tks.row_bits = row_bits;
    tks.nseg = (u32)std::min<u64>((cap + 4 * TPB - 1) / (4 * TPB), BIN_SEGS);
    const u64 wg_rows = ((cap + TK_TILE - 1) / TK_TILE + tks.nseg - 1) / tks.nseg * TK_TILE; // a workgroup takes whole tiles
    tks.segcap = c->bin_cap ? c->bin_cap : ((wg_rows / TP) * 3 / 2 + 64 + 15) / 16 * 16; // 1.5x an even share, whole 128-byte lines
    void *q[2];
    TRY(scratch(c, c->s_tk[0], TP * tks.nseg * tks.segcap * 8, &q[0]));
    TRY(scratch(c, c->s_tk[1], cap * 8, &q[1]));
    tks.tickets = (u64 *)q[0];
    tks.spill = (u64 *)q[1];
    if (!c->d_tk_meta) HIP_TRY(c, hipMalloc(&c->d_tk_meta, TK_META_HEAD + (size_t)TK_MAXP * BIN_SEGS * 4));
    tks.spill_count = c->d_tk_meta;
    tks.ablate = (u32)c->scan_ablate >> 8; // (timing-only diagnostics of pass one: scan_ablate 256, 512)
    tks.counts = (u32 *)((char *)c->d_tk_meta + TK_META_HEAD);
    *out = tks;
    return MG_OK;
}
// the partition form: the coarse gate's survivors binned by fine-gate slice, in segments for launch groups of up to `cap` rows
int bin_layout(mg_ctx *c, u64 cap, BinSet *out)
{
    BinSet bins{};
    const u64 P = ticket_slices(c);
    bins.nbins = (u32)P;
    bins.word_shift = (u32)(c->pregate_log2 - 1 - 6);
    bins.nseg = (u32)std::min<u64>((cap + 2 * TPB - 1) / (2 * TPB), BIN_SEGS);
    // 1.5x an even share of the worst case (every row passes the coarse gate)
    bins.segcap = c->bin_cap ? c->bin_cap : ((cap / P / bins.nseg) * 3 / 2 + 256 + 63) / 64 * 64; // line-aligned segments
    bins.ring = 64;
    while (bins.ring < 256 && bins.ring * 2 * P <= BIN_LDS_ROWS) bins.ring *= 2;
    if (c->bin_ring && (u64)c->bin_ring * P <= BIN_LDS_ROWS) bins.ring = (u32)c->bin_ring;
    void *q[6];
    for (int i = 0; i < 3; ++i) TRY(scratch(c, c->s_bin[i], P * bins.nseg * bins.segcap * (i == 2 ? 4 : 8), &q[i]));
    for (int i = 0; i < 3; ++i) TRY(scratch(c, c->s_spill[i], cap * (i == 2 ? 4 : 8), &q[3 + i]));
    bins.rows = RowList{(u64 *)q[0], (u64 *)q[1], (u32 *)q[2]};
    bins.spill = RowList{(u64 *)q[3], (u64 *)q[4], (u32 *)q[5]};
    if (!c->d_bin_meta) HIP_TRY(c, hipMalloc(&c->d_bin_meta, 8 + (size_t)BIN_MAXP * BIN_SEGS * 4));
    bins.spill_count = c->d_bin_meta;
    bins.counts = (u32 *)(c->d_bin_meta + 1);
    *out = bins;
    return MG_OK;
}
// ---- the sub-slice form's host side ---------------------------------------------------------------------------------------
constexpr int SCAN_EV_CHUNKS = 64; // launch groups of one scan whose kernels are timed (mg_scan_stats)
int device_cus(mg_ctx *c)
{
    if (!c->n_cus) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0) cus = 256;
        c->n_cus = cus;
    }
    return c->n_cus;
}
u64 sub_bins(const mg_ctx *c) // LDS-sized pieces (2^sub_words_log2 words) the fine gate splits into
{
    const u64 nwords = (c->bf[MG_BF_ALT].n_gate_bits + 63) / 64;
    return (nwords + (1ULL << c->sub_words_log2) - 1) >> c->sub_words_log2;
}
// segments, regions and meta block for launch groups of up to `cap` rows
int sub_layout(mg_ctx *c, u64 cap, u32 row_bits, SubSet *out)
{
    const BFState &alt = c->bf[MG_BF_ALT];
    SubSet ss{};
    const u64 NB = sub_bins(c);
    const int cus = device_cus(c);
    ss.nbins = (u32)NB;
    ss.words_log2 = (u32)c->sub_words_log2;
    ss.bin_shift = alt.gate_shift + 6 + ss.words_log2;
    ss.row_bits = row_bits;
    ss.n_gate_words = (alt.n_gate_bits + 63) / 64;
    const u64 tiles = (cap + SB_TILE - 1) / SB_TILE;
    ss.nseg = (u32)std::min<u64>(tiles, (u64)(c->sub_grid > 0 ? c->sub_grid : cus));
    const u64 wg_rows = (tiles + ss.nseg - 1) / ss.nseg * SB_TILE; // a workgroup takes whole tiles
    ss.segcap = c->bin_cap ? c->bin_cap : ((wg_rows / NB) * 3 / 2 + 64 + 15) / 16 * 16; // 1.5x an even share, whole 128-byte lines
    ss.parts = (u32)std::max<u64>(1, std::min<u64>(std::min<u64>(8, ss.nseg), (u64)cus / NB)); // bins fewer than CUs: several workgroups share one
    const u64 spp = (ss.nseg + ss.parts - 1) / ss.parts, units = NB * ss.parts;
    ss.ucap = spp * ss.segcap;
    void *q[4];
    TRY(scratch(c, c->s_sb[0], NB * ss.nseg * ss.segcap * 8, &q[0]));
    TRY(scratch(c, c->s_sb[1], cap * 8, &q[1]));
    TRY(scratch(c, c->s_sb[2], (units * ss.ucap + cap) * 8, &q[2]));
    const size_t head = (8 + (units + 1) * 4 + 15) / 16 * 16;
    TRY(scratch(c, c->s_sb[3], head + NB * ss.nseg * 4, &q[3]));
    ss.tickets = (u64 *)q[0];
    ss.spill = (u64 *)q[1];
    ss.out_tk = (u64 *)q[2];
    ss.spill_count = (unsigned long long *)q[3];
    ss.out_counts = (u32 *)((char *)q[3] + 8);
    ss.counts = (u32 *)((char *)q[3] + head);
    ss.ablate = (u32)c->scan_ablate >> 8; // (timing-only diagnostic of pass one: scan_ablate 256)
    *out = ss;
    return MG_OK;
}
// bytes of the meta block's head that every launch group starts from zero: the spill count and the regions' counts
size_t sub_meta_head(const SubSet &ss) { return 8 + ((size_t)ss.nbins * ss.parts + 1) * 4; }
// ---- one scan's plan ------------------------------------------------------------------------------------------------------
// the table a scan walks: the SoA arrays (hi, lo, cnt) or, when `rows12` is set, the compact 12-byte rows
struct ScanTable {
    const u64 *hi = nullptr, *lo = nullptr;
    const u32 *cnt = nullptr, *rows12 = nullptr;
    ScanTable from(u64 r0) const // the table from row r0 on (compact rows: r0 is a multiple of 4, a quad of rows is three 16-byte words)
    {
        return rows12 ? ScanTable{nullptr, nullptr, nullptr, rows12 + r0 / 4 * 12} : ScanTable{hi + r0, lo + r0, cnt + r0, nullptr};
    }
};
enum class ScanForm { direct, bins, tickets, subs };
// the form a scan takes, its rows per launch group, its two row lists and the form's layout
struct ScanPlan {
    ScanForm form = ScanForm::direct;
    u64 chunk = 0;
    RowList open{}, hits{};
    BinSet bins{};
    TicketSet tks{};
    SubSet subs{};
};
// The first form that fits the index: sub-slices of the gate answered out of LDS (whole-genome index), 2 MiB slices walked out
// of L2 (tickets), the coarse gate's survivors binned by slice (partition: SoA tables only), else the filter kernel alone.
int scan_plan(mg_ctx *c, u64 n, bool rows12, ScanPlan *out)
{
    ScanPlan p{};
    const BFState &alt = c->bf[MG_BF_ALT];
    u32 idx_bits = 1; // a ticket holds a filter index and the row number: rows per launch group = 2^row_bits
    while (idx_bits < 64 && (alt.size - 1) >> idx_bits) ++idx_bits;
    const u32 row_bits = std::min<u32>(27, 64 - idx_bits);
    const bool two_pass = c->use_summary && alt.gate && idx_bits <= 44 && !alt.gate_words; // (a gate sized in words is not cut into slices)
    const u64 NB = sub_bins(c), TP = ticket_slices(c);
    if (two_pass && c->use_sub && c->gate_log2 >= c->sub_min_log2 && NB >= 2 && NB <= (u64)SB_MAXB && c->sub_words_log2 >= 0 &&
        c->sub_words_log2 <= SB_WORDS_LOG2)
        p.form = ScanForm::subs;
    else if (two_pass && c->use_tickets && c->gate_log2 >= c->ticket_min_log2 && TP >= 2 && TP <= (u64)TK_MAXP)
        p.form = ScanForm::tickets;
    else if (!rows12 && alt.pregate && pregate_on(c) && c->use_summary && c->use_pregate && c->use_partition && TP >= 2 && TP <= BIN_MAXP)
        p.form = ScanForm::bins;
    const bool ticketed = p.form == ScanForm::tickets || p.form == ScanForm::subs;
    p.chunk = 1ULL << std::min<u32>(ticketed ? row_bits : 27, (u32)c->chunk_log2); // (bounds the two lists' worst-case size)
    if (rows12) p.chunk = std::max<u64>(4, p.chunk); // (a multiple of 4 rows: chunks start on whole quads)
    const u64 cap = n < p.chunk ? n : p.chunk; // worst case (gate disabled): every row is listed
    void *q[6];
    Scratch *sc[6] = {&c->s_open[0], &c->s_open[1], &c->s_open[2], &c->s_hit[0], &c->s_hit[1], &c->s_hit[2]};
    for (int i = 0; i < 6; ++i) TRY(scratch(c, *sc[i], cap * (i % 3 == 2 ? 4 : 8), &q[i]));
    p.open = RowList{(u64 *)q[0], (u64 *)q[1], (u32 *)q[2]};
    p.hits = RowList{(u64 *)q[3], (u64 *)q[4], (u32 *)q[5]};
    if (c->use_hit_entries && c->map.cap_log2 <= 30) { // (record * 2 + entry in 32 bits)
        void *pa;
        TRY(scratch(c, c->s_hit[3], cap * 8, &pa));
        p.hits.aux = (u64 *)pa;
    }
    if (p.form == ScanForm::tickets) TRY(ticket_layout(c, cap, row_bits, &p.tks));
    if (p.form == ScanForm::subs) TRY(sub_layout(c, cap, row_bits, &p.subs));
    if (p.form == ScanForm::bins) TRY(bin_layout(c, cap, &p.bins));
    *out = p;
    return MG_OK;
}
// the four events of launch group `chunk` of the running scan (created on first use); nullptr beyond SCAN_EV_CHUNKS, and from the
// first group whose events could not be made on (ev_rows only ever lists groups with all four events)
hipEvent_t *scan_events(mg_ctx *c, u64 chunk, u64 rows)
{
    if (chunk >= (u64)SCAN_EV_CHUNKS || chunk != c->ev_rows.size()) return nullptr;
    while (c->ev.size() < 4 * (chunk + 1)) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        c->ev.push_back(e);
    }
    c->ev_rows.push_back(rows);
    return c->ev.data() + 4 * chunk;
}
// ---- one launch group ------------------------------------------------------------------------------------------------------
template <int KC, int RC>
void launch_sub_passes(mg_ctx *c, const u64 *d_hi, const u64 *d_lo, const u32 *rows12, u64 n, const SubSet &layout)
{
    SubSet ss = layout;
    ss.nseg = (u32)std::min<u64>((n + SB_TILE - 1) / SB_TILE, layout.nseg); // (regions and segments stay as laid out: a smaller grid fills fewer of them)
    const BFView alt = view(c, MG_BF_ALT);
    if (rows12) hipLaunchKernelGGL((scan_sub_sort_kernel<KC, RC, true>), dim3(ss.nseg), dim3(SB_TPB), 0, c->stream, d_hi, d_lo, rows12, n, (int)c->k, (int)c->ref_k, alt, ss);
    else hipLaunchKernelGGL((scan_sub_sort_kernel<KC, RC, false>), dim3(ss.nseg), dim3(SB_TPB), 0, c->stream, d_hi, d_lo, rows12, n, (int)c->k, (int)c->ref_k, alt, ss);
    const unsigned units = ss.nbins * ss.parts;
    const unsigned grid = std::min<unsigned>(units, (unsigned)device_cus(c));
    if (c->gate_k == 4) hipLaunchKernelGGL(scan_sub_gate_kernel<4>, dim3(grid), dim3(SB_TPB), 0, c->stream, alt, ss);
    else hipLaunchKernelGGL(scan_sub_gate_kernel<0>, dim3(grid), dim3(SB_TPB), 0, c->stream, alt, ss);
    hipLaunchKernelGGL(sub_total_kernel, dim3(1), dim3(SB_TPB), 0, c->stream, (const u32 *)ss.out_counts, units + 1, c->d_hit_count);
}
template <int KC, int RC, int ROWS, int VAR>
void launch_filter_var(mg_ctx *c, const u64 *d_hi, const u64 *d_lo, const u32 *d_cnt, u64 n, RowList open)
{
    const u64 per_block = (u64)TPB * ROWS;
    const unsigned grid = (unsigned)std::min<u64>((n + per_block - 1) / per_block, (u64)c->scan_grid);
    hipLaunchKernelGGL((scan_filter_kernel<KC, RC, ROWS, VAR>), dim3(grid), dim3(TPB), 0, c->stream, d_hi, d_lo, d_cnt, n, (int)c->k,
                       (int)c->ref_k, view(c, MG_BF_ALT), open, c->d_hit_count, c->scan_ablate);
}
template <int KC, int RC, int ROWS>
void launch_filter_rows(mg_ctx *c, const u64 *d_hi, const u64 *d_lo, const u32 *d_cnt, u64 n, RowList open)
{
    // 16-byte loads need 16-byte aligned table bases (chunk offsets are multiples of 2^27 rows, so only the caller's bases matter)
    const bool vec_ok = ROWS == 2 && ((((uintptr_t)d_hi | (uintptr_t)d_lo) & 15) == 0) && (((uintptr_t)d_cnt & 7) == 0);
    switch ((c->scan_variant & 2) && vec_ok ? 2 : 0) {
    case 2: launch_filter_var<KC, RC, ROWS, 2>(c, d_hi, d_lo, d_cnt, n, open); break;
    default: launch_filter_var<KC, RC, ROWS, 0>(c, d_hi, d_lo, d_cnt, n, open); break;
    }
}
// The two passes of the ticket form over one chunk of the table (SoA arrays, or compact rows when `rows12` is given).
template <int KC, int RC>
void launch_ticket_passes(mg_ctx *c, const u64 *d_hi, const u64 *d_lo, const u32 *rows12, u64 n, const TicketSet &layout, RowList open)
{
    TicketSet ts = layout;
    ts.nseg = (u32)std::min<u64>((n + 4 * TPB - 1) / (4 * TPB), layout.nseg);
    hipLaunchKernelGGL((scan_ticket_sort_kernel<KC, RC>), dim3(ts.nseg), dim3(TPB), 0, c->stream, d_hi, d_lo, rows12, n, (int)c->k, (int)c->ref_k,
                       view(c, MG_BF_ALT), ts);
    if (!c->tkg_grid) c->tkg_grid = std::max(8, device_cus(c) / 8 * 8); // pass two walks the slices in step: one workgroup per CU, all resident together
    if (c->gate_k == 4)
        hipLaunchKernelGGL(scan_ticket_gate_kernel<4>, dim3(c->tkg_grid), dim3(TKG_TPB), 0, c->stream, view(c, MG_BF_ALT), ts, open.cnt, c->d_hit_count);
    else
        hipLaunchKernelGGL(scan_ticket_gate_kernel<0>, dim3(c->tkg_grid), dim3(TKG_TPB), 0, c->stream, view(c, MG_BF_ALT), ts, open.cnt, c->d_hit_count);
}
constexpr u32 ROWS12_MAX_R = 44; // compact rows hold a ref_k-mer of 33..44 bases and a count of 96 - 2 ref_k bits
int rows12_ok(mg_ctx *c)
{
    if (c->ref_k < 33 || c->ref_k > ROWS12_MAX_R)
        return fail(c, MG_ERR_LIMIT, "packed 12-byte rows hold a ref_k-mer of 33..44 bases and a count of 96 - 2 ref_k bits (ref_k = %u): use the SoA table", c->ref_k);
    return MG_OK;
}
// One launch group of a scan: its form's passes, then (but for the sub-slice form, whose probe kernel is its hit pass too) the
// probe and hit kernels over the two row lists.  ev: the group's four events, or NULL.
template <int KC, int RC>
void launch_scan_chunk(mg_ctx *c, const ScanTable &t, u64 n, const ScanPlan &p, hipEvent_t *ev)
{
    if (ev) hipEventRecord(ev[0], c->stream);
    switch (p.form) {
    case ScanForm::subs: { // whole-genome index: tickets filed by LDS-sized sub-slice of the gate, then each sub-slice answered out of LDS
        launch_sub_passes<KC, RC>(c, t.hi, t.lo, t.rows12, n, p.subs);
        if (ev) hipEventRecord(ev[1], c->stream);
        // regions of surviving tickets: the record first, the table row where the record asks for it
        const SubSet &ss = p.subs;
        const SubOpen so{ss.out_counts, ss.out_tk, ss.ucap, ss.nbins * ss.parts + 1, (u32)std::max(1, c->sub_split), ss.row_bits};
        const unsigned pgrid = std::min<unsigned>(so.n_units * so.split, 2 * (unsigned)c->probe_grid);
        hipLaunchKernelGGL((scan_sub_probe_kernel<KC, RC>), dim3(pgrid), dim3(TPB), 0, c->stream, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c, MG_BF_CTX), view(c), so,
                           c->d_hit_count, t.cnt, t.hi, t.lo, t.rows12);
        if (ev) hipEventRecord(ev[2], c->stream);
        if (ev) hipEventRecord(ev[3], c->stream);
        return;
    }
    case ScanForm::tickets: // the same with 2 MiB slices walked out of L2; the open list holds row numbers
        launch_ticket_passes<KC, RC>(c, t.hi, t.lo, t.rows12, n, p.tks, p.open);
        break;
    case ScanForm::bins: { // large index: coarse gate + binning, then the fine gate slice by slice
        BinSet bs = p.bins; // the last chunk may need fewer workgroups than segments were laid out for
        bs.nseg = (u32)std::min<u64>((n + 2 * TPB - 1) / (2 * TPB), p.bins.nseg);
        if (c->bin_rows == 4)
            hipLaunchKernelGGL((scan_bin_kernel<KC, RC, 4>), dim3(bs.nseg), dim3(TPB), (size_t)bs.nbins * bs.ring * 20, c->stream, t.hi, t.lo, t.cnt, n,
                               (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), bs, c->scan_ablate);
        else
            hipLaunchKernelGGL((scan_bin_kernel<KC, RC, 2>), dim3(bs.nseg), dim3(TPB), (size_t)bs.nbins * bs.ring * 20, c->stream, t.hi, t.lo, t.cnt, n,
                               (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), bs, c->scan_ablate);
        hipLaunchKernelGGL((scan_bin_gate_kernel<KC, RC>), dim3(2048), dim3(TPB), 0, c->stream, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT),
                           bs, p.open, c->d_hit_count);
        break;
    }
    case ScanForm::direct:
        if (t.rows12) {
            if constexpr (RC <= (int)ROWS12_MAX_R) { // (no compact-row instance for a longer fixed ref_k: rows12_ok keeps those tables out)
                const unsigned fgrid = (unsigned)std::min<u64>(((n + 1) / 2 + TPB - 1) / TPB, (u64)c->scan_grid);
                hipLaunchKernelGGL((scan_filter12_kernel<KC, RC>), dim3(fgrid), dim3(TPB), 0, c->stream, t.rows12, n, (int)c->k, (int)c->ref_k,
                                   view(c, MG_BF_ALT), p.open, c->d_hit_count, c->scan_ablate);
            }
        } else
            switch (c->scan_rows) {
            case 1: launch_filter_rows<KC, RC, 1>(c, t.hi, t.lo, t.cnt, n, p.open); break;
            case 4: launch_filter_rows<KC, RC, 4>(c, t.hi, t.lo, t.cnt, n, p.open); break;
            default: launch_filter_rows<KC, RC, 2>(c, t.hi, t.lo, t.cnt, n, p.open); break;
            }
        break;
    }
    if (ev) hipEventRecord(ev[1], c->stream);
    // the list lengths live on the device; fixed grids walk them with a stride, so no host round trip.  The lists hold the rows, but for
    // the direct form over SoA arrays (the row's index: the probe fetches its count) and the ticket form (row numbers: it fetches the row)
    const bool tk = p.form == ScanForm::tickets;
    const unsigned grid = (unsigned)std::min<u64>(nblocks(n), (u64)c->probe_grid);
    hipLaunchKernelGGL((scan_probe_kernel<KC, RC>), dim3(grid), dim3(TPB), 0, c->stream, (int)c->k, (int)c->ref_k, view(c, MG_BF_ALT), view(c), p.open, p.hits,
                       c->d_hit_count, p.form == ScanForm::bins ? nullptr : t.cnt, tk ? t.hi : nullptr, tk ? t.lo : nullptr, tk ? t.rows12 : nullptr);
    if (ev) hipEventRecord(ev[2], c->stream);
    hipLaunchKernelGGL((scan_hits_kernel<KC, RC>), dim3(std::min(grid, (unsigned)c->hits_grid)), dim3(TPB), 0, c->stream, (int)c->k, (int)c->ref_k,
                       view(c, MG_BF_ALT), view(c, MG_BF_CTX), view(c), p.hits, c->d_hit_count);
    if (ev) hipEventRecord(ev[3], c->stream);
}
// A scan of a device-resident table (after the entry point's argument checks), in launch groups of plan.chunk rows
int scan_table(mg_ctx *c, const ScanTable &t, u64 n)
{
    if (!c->map.slots) TRY(map_reserve(c, 0));
    TRY(ctx_set_ready(c));
    TRY(records_current(c));
    c->stats_valid = false;
    c->ev_rows.clear();
    ScanPlan p;
    TRY(scan_plan(c, n, t.rows12 != nullptr, &p));
    HIP_TRY(c, hipMemsetAsync(c->d_hit_count, 0, 32, c->stream));
    for (u64 r0 = 0; r0 < n; r0 += p.chunk) {
        const u64 nr = n - r0 < p.chunk ? n - r0 : p.chunk;
        if (r0) HIP_TRY(c, hipMemsetAsync(c->d_hit_count, 0, 16, c->stream));
        if (p.form == ScanForm::bins) HIP_TRY(c, hipMemsetAsync(c->d_bin_meta, 0, 8, c->stream));
        if (p.form == ScanForm::tickets) HIP_TRY(c, hipMemsetAsync(c->d_tk_meta, 0, TK_META_HEAD, c->stream));
        if (p.form == ScanForm::subs) HIP_TRY(c, hipMemsetAsync(p.subs.spill_count, 0, sub_meta_head(p.subs), c->stream));
        hipEvent_t *ev = scan_events(c, r0 / p.chunk, nr);
        const ScanTable tc = t.from(r0);
        // the reference's defaults (k35 r43, argument_parser.hpp:57-58) and config C5 (k35 r63: SoA tables only) get fixed-length hashing
        if (c->k == 35 && c->ref_k == 43) launch_scan_chunk<35, 43>(c, tc, nr, p, ev);
        else if (c->k == 35 && c->ref_k == 63) launch_scan_chunk<35, 63>(c, tc, nr, p, ev);
        else launch_scan_chunk<0, 0>(c, tc, nr, p, ev);
        HIP_TRY(c, hipGetLastError());
    }
    c->last_bins = p.form == ScanForm::bins ? (int)p.bins.nbins : 0;
    c->last_tickets = p.form == ScanForm::tickets ? (int)p.tks.nbins : 0;
    c->last_subs = p.form == ScanForm::subs ? (int)p.subs.nbins : 0;
    if (p.form == ScanForm::subs && view(c).lazy) c->vec_stale = true; // (the records' copies are ahead of the vectors now)
    else c->vec_zero = false;
    c->stats_valid = true;
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_kmc_scan_device(mg_ctx *c, const void *d_hi, const void *d_lo, const void *d_cnt, size_t n)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->bf[0].mode || !c->bf[1].mode) return fail(c, MG_ERR_STATE, "mg_kmc_scan needs both filters finalised");
    if (c->ref_k > MG_MAX_PACKED_K)
        return fail(c, MG_ERR_LIMIT, "packed scan supports k <= ref_k <= 64 (k=%u ref_k=%u)", c->k, c->ref_k);
    if (n == 0) return MG_OK;
    if (!d_hi || !d_lo || !d_cnt) return fail(c, MG_ERR_ARG, "NULL table pointer");
    return scan_table(c, ScanTable{(const u64 *)d_hi, (const u64 *)d_lo, (const u32 *)d_cnt, nullptr}, n);
}

// ---- compact (12-byte) table rows --------------------------------------------------------------------------------

MG_EXPORT size_t mg_kmc_rows_bytes(size_t n) { return (n + 3) / 4 * 4 * 12; }

MG_EXPORT int mg_kmc_pack_rows_device(mg_ctx *c, const void *d_hi, const void *d_lo, const void *d_cnt, size_t n, void *d_rows_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(rows12_ok(c));
    if (n == 0) return MG_OK;
    if (!d_hi || !d_lo || !d_cnt || !d_rows_out) return fail(c, MG_ERR_ARG, "NULL pointer");
    int *d_bad = (int *)(c->d_hit_count + 3);
    HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
    hipLaunchKernelGGL(pack_rows12_kernel, dim3(nblocks((n + 3) / 4 * 4)), dim3(TPB), 0, c->stream, (const u64 *)d_hi, (const u64 *)d_lo, (const u32 *)d_cnt,
                       (u64)n, (int)c->ref_k, (u32 *)d_rows_out, d_bad);
    HIP_TRY(c, hipGetLastError());
    int bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bad) return fail(c, MG_ERR_LIMIT, "a count of 2^%u or more (or a k-mer wider than ref_k) does not fit a packed row: use the SoA table", 96 - 2 * c->ref_k);
    return MG_OK;
}

MG_EXPORT int mg_kmc_scan_rows_device(mg_ctx *c, const void *d_rows, size_t n)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->bf[0].mode || !c->bf[1].mode) return fail(c, MG_ERR_STATE, "mg_kmc_scan needs both filters finalised");
    TRY(rows12_ok(c));
    if (n == 0) return MG_OK;
    if (!d_rows || ((uintptr_t)d_rows & 15)) return fail(c, MG_ERR_ARG, "packed rows must be 16-byte aligned");
    return scan_table(c, ScanTable{nullptr, nullptr, nullptr, (const u32 *)d_rows}, n);
}

namespace {
// Host-fed scans stream the table through the device in pieces.  Two staging slots: while the scan kernels work
// on one, the copy stream fills the other (PCIe and HBM work overlap; with pinned host memory -- mg_host_alloc --
// the copies are truly asynchronous, with pageable memory the runtime stages them and the host blocks per copy,
// which still leaves the previous piece's kernels running underneath).
int pipeline_ready(mg_ctx *c)
{
    if (c->copy_stream) return MG_OK;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_up[i], hipEventDisableTiming));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_free[i], hipEventDisableTiming));
    }
    return MG_OK;
}
constexpr size_t HOST_PIECE = 1u << 24; // rows per staged piece: 320 MB of SoA rows per slot
// Host-fed scans leave DMA from the caller's buffers in flight on copy_stream: whatever way the call ends, both streams are
// drained before the caller (who may free or unmap the source on an error) sees the result.
struct StreamsDrained {
    mg_ctx *c;
    ~StreamsDrained()
    {
        if (c->copy_stream) hipStreamSynchronize(c->copy_stream);
        hipStreamSynchronize(c->stream);
    }
};
// The two-slot loop of a host-fed scan, HOST_PIECE rows at a time: `upload(slot, r0, nr, d)` queues the piece's copies on
// copy_stream, `decode(slot, r0, nr, d)` what turns them into the SoA rows d[0..2] on the scan stream, and the rows are scanned.
template <class Upload, class Decode>
int scan_host_pieces(mg_ctx *c, size_t n, Upload upload, Decode decode)
{
    TRY(pipeline_ready(c));
    const StreamsDrained drained{c};
    const size_t cap = n < HOST_PIECE ? n : HOST_PIECE;
    void *d[2][3];
    for (int sl = 0; sl < 2; ++sl)
        for (int i = 0; i < 3; ++i) TRY(scratch(c, c->s_stage[sl][i], cap * (i == 2 ? 4 : 8), &d[sl][i]));
    size_t piece_no = 0;
    for (size_t r0 = 0; r0 < n; r0 += HOST_PIECE, ++piece_no) {
        const size_t nr = n - r0 < HOST_PIECE ? n - r0 : HOST_PIECE;
        const int sl = (int)(piece_no & 1);
        if (piece_no >= 2) HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_free[sl], 0)); // the scan that used this slot is done
        TRY(upload(sl, r0, nr, d[sl]));
        HIP_TRY(c, hipEventRecord(c->ev_up[sl], c->copy_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_up[sl], 0));
        TRY(decode(sl, r0, nr, d[sl]));
        TRY(mg_kmc_scan_device(c, d[sl][0], d[sl][1], d[sl][2], nr));
        HIP_TRY(c, hipEventRecord(c->ev_free[sl], c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the caller may reuse its buffers
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_kmc_scan(mg_ctx *c, const uint64_t *hi, const uint64_t *lo, const uint32_t *cnt, size_t n)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    if (!hi || !lo || !cnt) return fail(c, MG_ERR_ARG, "NULL table pointer");
    if (!c->bf[0].mode || !c->bf[1].mode) return fail(c, MG_ERR_STATE, "mg_kmc_scan needs both filters finalised");
    const auto upload = [&](int, size_t r0, size_t nr, void *const *d) -> int {
        HIP_TRY(c, hipMemcpyAsync(d[0], hi + r0, nr * 8, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(c, hipMemcpyAsync(d[1], lo + r0, nr * 8, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(c, hipMemcpyAsync(d[2], cnt + r0, nr * 4, hipMemcpyHostToDevice, c->copy_stream));
        return MG_OK;
    };
    return scan_host_pieces(c, n, upload, [](int, size_t, size_t, void *const *) -> int { return MG_OK; });
}

// ---- KMC database feed -------------------------------------------------------------------------

MG_EXPORT int mg_host_alloc(void **out, size_t bytes)
{
    if (!out) return MG_ERR_ARG;
    *out = nullptr;
    return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? MG_OK : MG_ERR_NOMEM;
}
MG_EXPORT int mg_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) return MG_ERR_HIP;
    return MG_OK;
}

MG_EXPORT int mg_kmc_set_lut(mg_ctx *c, const uint64_t *lut, size_t n_lut, uint32_t lut_prefix_len, uint32_t suffix_bytes,
                             uint32_t counter_bytes, uint32_t min_count, uint64_t max_count, uint64_t total_records)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (!lut || n_lut == 0) return fail(c, MG_ERR_ARG, "mg_kmc_set_lut: empty prefix table");
    if (lut_prefix_len == 0 || lut_prefix_len > 15) return fail(c, MG_ERR_ARG, "mg_kmc_set_lut: lut_prefix_len %u (1..15)", lut_prefix_len);
    if (counter_bytes < 1 || counter_bytes > 4) return fail(c, MG_ERR_LIMIT, "KMC counters of %u bytes (1..4 supported: the reference reads them into a uint32)", counter_bytes);
    if (suffix_bytes < 1 || suffix_bytes > 15 || lut_prefix_len + 4 * suffix_bytes != c->ref_k)
        return fail(c, MG_ERR_ARG, "database k = %u (prefix %u + %u suffix bytes), context expects -r %u", lut_prefix_len + 4 * suffix_bytes,
                    lut_prefix_len, suffix_bytes, c->ref_k);
    if (c->ref_k > MG_MAX_PACKED_K) return fail(c, MG_ERR_LIMIT, "packed scan supports ref_k <= 64");
    if (n_lut % (1ULL << (2 * lut_prefix_len)) != 0) return fail(c, MG_ERR_ARG, "prefix table of %zu entries is not a whole number of 4^%u-entry bins", n_lut, lut_prefix_len);
    if (lut[0] != 0) return fail(c, MG_ERR_ARG, "prefix table does not start at record 0");
    for (size_t j = 1; j < n_lut; ++j)
        if (lut[j] < lut[j - 1] || lut[j] > total_records) return fail(c, MG_ERR_ARG, "prefix table is not ascending within the %llu records", (unsigned long long)total_records);
    hipFree(c->d_kmc_lut);
    c->d_kmc_lut = nullptr;
    HIP_TRY(c, hipMalloc(&c->d_kmc_lut, (n_lut + 1) * 8));
    HIP_TRY(c, hipMemcpy(c->d_kmc_lut, lut, n_lut * 8, hipMemcpyHostToDevice));
    const u64 guard = ~0ULL; // above every record index
    HIP_TRY(c, hipMemcpy(c->d_kmc_lut + n_lut, &guard, 8, hipMemcpyHostToDevice));
    c->kmc_n_lut = n_lut;
    c->kmc_prefix_len = lut_prefix_len;
    c->kmc_suffix_bytes = suffix_bytes;
    c->kmc_counter_bytes = counter_bytes;
    c->kmc_min_count = min_count;
    c->kmc_max_count = max_count;
    return MG_OK;
}

MG_EXPORT int mg_kmc_scan_records(mg_ctx *c, const void *records, size_t n, uint64_t first_record)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    if (!records) return fail(c, MG_ERR_ARG, "NULL records");
    if (!c->d_kmc_lut) return fail(c, MG_ERR_STATE, "mg_kmc_set_lut first");
    if (!c->bf[0].mode || !c->bf[1].mode) return fail(c, MG_ERR_STATE, "mg_kmc_scan needs both filters finalised");
    const size_t rs = c->kmc_suffix_bytes + c->kmc_counter_bytes;
    void *raw[2];
    for (int sl = 0; sl < 2; ++sl) TRY(scratch(c, c->s_raw[sl], (n < HOST_PIECE ? n : HOST_PIECE) * rs + 64, &raw[sl]));
    const auto upload = [&](int sl, size_t r0, size_t nr, void *const *) -> int {
        HIP_TRY(c, hipMemcpyAsync(raw[sl], (const char *)records + r0 * rs, nr * rs, hipMemcpyHostToDevice, c->copy_stream));
        return MG_OK;
    };
    const auto decode = [&](int sl, size_t r0, size_t nr, void *const *d) -> int {
        hipLaunchKernelGGL(kmc_decode_kernel, dim3((unsigned)((nr + KMC_TILE - 1) / KMC_TILE)), dim3(TPB), 0, c->stream, (const u8 *)raw[sl], (u64)nr,
                           (u64)(first_record + r0), c->kmc_suffix_bytes, c->kmc_counter_bytes, c->kmc_prefix_len, (const u64 *)c->d_kmc_lut, c->kmc_n_lut,
                           c->kmc_min_count, c->kmc_max_count, (u64 *)d[0], (u64 *)d[1], (u32 *)d[2]);
        HIP_TRY(c, hipGetLastError());
        return MG_OK;
    };
    return scan_host_pieces(c, n, upload, decode);
}

// the decoded rows of a run of records (tests, and callers that want the table itself)
MG_EXPORT int mg_kmc_decode_records(mg_ctx *c, const void *records, size_t n, uint64_t first_record, uint64_t *hi_out, uint64_t *lo_out,
                                    uint32_t *cnt_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n == 0) return MG_OK;
    if (!records || !hi_out || !lo_out || !cnt_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!c->d_kmc_lut) return fail(c, MG_ERR_STATE, "mg_kmc_set_lut first");
    const size_t rs = c->kmc_suffix_bytes + c->kmc_counter_bytes;
    for (size_t r0 = 0; r0 < n; r0 += HOST_PIECE) {
        const size_t nr = n - r0 < HOST_PIECE ? n - r0 : HOST_PIECE;
        void *d[3], *raw;
        for (int i = 0; i < 3; ++i) TRY(scratch(c, c->s_stage[0][i], nr * (i == 2 ? 4 : 8), &d[i]));
        TRY(scratch(c, c->s_raw[0], nr * rs + 64, &raw));
        HIP_TRY(c, hipMemcpyAsync(raw, (const char *)records + r0 * rs, nr * rs, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(kmc_decode_kernel, dim3((unsigned)((nr + KMC_TILE - 1) / KMC_TILE)), dim3(TPB), 0, c->stream, (const u8 *)raw, (u64)nr,
                           (u64)(first_record + r0), c->kmc_suffix_bytes, c->kmc_counter_bytes, c->kmc_prefix_len, (const u64 *)c->d_kmc_lut, c->kmc_n_lut,
                           c->kmc_min_count, c->kmc_max_count, (u64 *)d[0], (u64 *)d[1], (u32 *)d[2]);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(hi_out + r0, d[0], nr * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(lo_out + r0, d[1], nr * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cnt_out + r0, d[2], nr * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return MG_OK;
}

MG_EXPORT int mg_scan_stats(mg_ctx *c, float *ms_out, uint64_t *n_hits)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->stats_valid || c->ev_rows.empty()) return fail(c, MG_ERR_STATE, "no scan has run");
    // per launch group (chunk) of the most recent scan, AVERAGED over its chunks by rows: the sums of the three phases over all
    // timed chunks, scaled to the rows of the first (largest) one -- what a rocprofv3 --stats average of the same kernels gives
    // when every chunk is full, and the same rate when the last one is not
    const size_t nc = c->ev_rows.size();
    HIP_TRY(c, hipEventSynchronize(c->ev[4 * nc - 1]));
    if (ms_out) {
        double sum[3] = {0, 0, 0};
        u64 rows = 0;
        for (size_t q = 0; q < nc; ++q) {
            for (int i = 0; i < 3; ++i) {
                float ms = 0;
                HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[4 * q + i], c->ev[4 * q + i + 1]));
                sum[i] += ms;
            }
            rows += c->ev_rows[q];
        }
        for (int i = 0; i < 3; ++i) ms_out[i] = (float)(sum[i] * (double)c->ev_rows[0] / (double)(rows ? rows : 1));
    }
    if (n_hits) {
        unsigned long long t[4] = {0, 0, 0, 0};
        HIP_TRY(c, hipMemcpy(t, c->d_hit_count, 32, hipMemcpyDeviceToHost));
        n_hits[0] = t[0]; // open rows of the last chunk
        n_hits[1] = t[2]; // bf hit rows of the whole call
    }
    return MG_OK;
}

MG_EXPORT int mg_debug_packed_index(mg_ctx *c, int which, const uint64_t *hi, const uint64_t *lo, size_t n, uint32_t klen,
                                    uint64_t *out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    if (klen < 1 || klen > MG_MAX_PACKED_K) return fail(c, MG_ERR_LIMIT, "packed k-mers: 1 <= k <= 64");
    if (n == 0) return MG_OK;
    void *dh, *dl, *dout;
    TRY(upload(c, c->s_misc[5], hi, n * 8, &dh));
    TRY(upload(c, c->s_misc[6], lo, n * 8, &dl));
    TRY(scratch(c, c->s_out, n * 8, &dout));
    hipLaunchKernelGGL(packed_index_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const u64 *)dh, (const u64 *)dl,
                       (u64)n, (int)klen, c->bf[which].mod, (u64 *)dout);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, dout, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// ---- counters exchange --------------------------------------------------------------------

MG_EXPORT int mg_counters_size(mg_ctx *c, uint64_t *n_bf, uint64_t *n_map)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    if (n_bf) *n_bf = c->bf[0].nset;
    if (n_map) *n_map = c->map.rows_total;
    return MG_OK;
}
namespace {
// the two counter arrays as ONE allocation [bf counters | map counters] (what an in-place all-reduce wants)
int ensure_joined(mg_ctx *c)
{
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    BFState &b = c->bf[MG_BF_ALT];
    MapState &m = c->map;
    if (!c->joined) {
        const u64 nb = b.nset, nm = m.rows_total;
        u32 *j = nullptr;
        HIP_TRY(c, hipMalloc(&j, (nb + nm ? nb + nm : 1) * 4));
        if (nb) HIP_TRY(c, hipMemcpyAsync(j, b.counts, nb * 4, hipMemcpyDeviceToDevice, c->stream));
        if (nm) HIP_TRY(c, hipMemcpyAsync(j + nb, m.vals, nm * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        hipFree(b.counts);
        hipFree(m.vals);
        c->joined = j;
        b.counts = j;
        m.vals = j + nb;
        m.vals_cap = nm;
    }
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_counters_view(mg_ctx *c, void **d_ptr, uint64_t *n_bf, uint64_t *n_map)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c || !d_ptr) return MG_ERR_ARG;
    TRY(ensure_joined(c));
    c->rec_off = true; // the caller may write the vector (an all-reduce by other means): from here on it alone holds the counters
    *d_ptr = c->joined;
    if (n_bf) *n_bf = c->bf[MG_BF_ALT].nset;
    if (n_map) *n_map = c->map.rows_total;
    return MG_OK;
}
namespace {
// one plane of a sample-minor counter vector (cohort mode): cell i of the plane at cells[i << shift]
__global__ void __launch_bounds__(TPB) plane_gather_kernel(const u32 *__restrict__ cells, u32 shift, u64 n, u32 *__restrict__ out)
{
    const u64 i = (u64)blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = cells[i << shift];
}
__global__ void __launch_bounds__(TPB) plane_scatter_kernel(u32 *__restrict__ cells, u32 shift, u64 n, const u32 *__restrict__ in)
{
    const u64 i = (u64)blockIdx.x * TPB + threadIdx.x;
    if (i < n) cells[i << shift] = in[i];
}
__global__ void __launch_bounds__(TPB) plane_zero_kernel(u32 *__restrict__ cells, u32 shift, u64 n)
{
    const u64 i = (u64)blockIdx.x * TPB + threadIdx.x;
    if (i < n) cells[i << shift] = 0u;
}
// the selected plane of the two vectors, gathered to d_bf / d_map (either may be NULL)
int plane_gather(mg_ctx *c, u32 *d_bf, u32 *d_map)
{
    const u64 nb = c->bf[0].mode ? c->bf[0].nset : 0, nm = c->map.rows_total;
    if (d_bf && nb) hipLaunchKernelGGL(plane_gather_kernel, dim3(nblocks(nb)), dim3(TPB), 0, c->stream, (const u32 *)c->bf[0].counts + c->coh_sel, c->coh_shift, nb, d_bf);
    if (d_map && nm) hipLaunchKernelGGL(plane_gather_kernel, dim3(nblocks(nm)), dim3(TPB), 0, c->stream, (const u32 *)c->map.vals + c->coh_sel, c->coh_shift, nm, d_map);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
} // namespace
MG_EXPORT int mg_counters_export_device(mg_ctx *c, void *d_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || !d_out) return MG_ERR_ARG;
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    const u64 nb = c->bf[0].nset, nm = c->map.rows_total;
    if (c->coh_planes) return plane_gather(c, (u32 *)d_out, (u32 *)d_out + nb);
    if (nb) HIP_TRY(c, hipMemcpyAsync(d_out, c->bf[0].counts, nb * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nm) HIP_TRY(c, hipMemcpyAsync((u32 *)d_out + nb, c->map.vals, nm * 4, hipMemcpyDeviceToDevice, c->stream));
    return MG_OK;
}
MG_EXPORT int mg_counters_import_device(mg_ctx *c, const void *d_in)
{
    const DeviceGuard on_device(c);
    if (!c || !d_in) return MG_ERR_ARG;
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    const u64 nb = c->bf[0].nset, nm = c->map.rows_total;
    if (c->coh_planes) {
        if (nb) hipLaunchKernelGGL(plane_scatter_kernel, dim3(nblocks(nb)), dim3(TPB), 0, c->stream, c->bf[0].counts + c->coh_sel, c->coh_shift, nb, (const u32 *)d_in);
        if (nm) hipLaunchKernelGGL(plane_scatter_kernel, dim3(nblocks(nm)), dim3(TPB), 0, c->stream, c->map.vals + c->coh_sel, c->coh_shift, nm, (const u32 *)d_in + nb);
        HIP_TRY(c, hipGetLastError());
        return MG_OK;
    }
    if (nb) HIP_TRY(c, hipMemcpyAsync(c->bf[0].counts, d_in, nb * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nm) HIP_TRY(c, hipMemcpyAsync(c->map.vals, (const u32 *)d_in + nb, nm * 4, hipMemcpyDeviceToDevice, c->stream));
    return MG_OK;
}
MG_EXPORT int mg_counters_reset(mg_ctx *c)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (c->coh_planes) { // the selected plane alone; the records hold no copies in cohort mode
        const u64 nb = c->bf[0].mode ? c->bf[0].nset : 0, nm = c->map.rows_total;
        if (nb) hipLaunchKernelGGL(plane_zero_kernel, dim3(nblocks(nb)), dim3(TPB), 0, c->stream, c->bf[0].counts + c->coh_sel, c->coh_shift, nb);
        if (nm) hipLaunchKernelGGL(plane_zero_kernel, dim3(nblocks(nm)), dim3(TPB), 0, c->stream, c->map.vals + c->coh_sel, c->coh_shift, nm);
        HIP_TRY(c, hipGetLastError());
        for (auto &kv : c->map.irregular) kv.second = 0;
        return MG_OK;
    }
    if (!c->vec_zero) { // (vectors that nothing has written since the last reset -- lazy scans only -- are still all zero)
        if (c->bf[0].mode && c->bf[0].nset) HIP_TRY(c, hipMemsetAsync(c->bf[0].counts, 0, c->bf[0].nset * 4, c->stream));
        if (c->map.rows_total) HIP_TRY(c, hipMemsetAsync(c->map.vals, 0, c->map.rows_total * 4, c->stream));
    }
    c->vec_zero = !c->joined && !c->rec_off; // (a vector that has been handed out may be written behind the library's back)
    c->vec_stale = false;                    // (whatever the records were ahead by is gone with their epoch)
    for (auto &kv : c->map.irregular) kv.second = 0;
    // every record's copy is now of an older epoch: it reads as zero, like the vectors just cleared.  At the wrap of the 32-bit
    // epoch the copies written 2^32 resets ago would read as current again: the next scan republishes every record instead
    // (records_current rewrites all of them from the vectors, which are zero)
    if (++c->rec_epoch == 0) {
        c->rec_epoch = 1;
        c->rec_ok = false;
    } else
        c->rec_ok = records_wanted(c) && c->map.slots != nullptr;
    return MG_OK;
}

// ---- cohort mode: the counters of several samples side by side ---------------------------------
// No counterpart in the reference, which runs the whole `call` (main.cpp:421-594) once per sample.
MG_EXPORT int mg_cohort_begin(mg_ctx *c, uint32_t n_planes)
{
    const DeviceGuard on_device(c); // (vectors brought up to date; the records' copies are invalid from here on)
    if (!c) return MG_ERR_ARG;
    if (n_planes < 1 || n_planes > 64) return fail(c, MG_ERR_ARG, "mg_cohort_begin: 1 <= n_planes <= 64 (got %u)", n_planes);
    if (c->coh_planes) return fail(c, MG_ERR_STATE, "mg_cohort_begin: already in cohort mode (%u planes)", c->coh_planes);
    if (!c->bf[MG_BF_ALT].mode || !c->bf[MG_BF_CTX].mode) return fail(c, MG_ERR_STATE, "mg_cohort_begin: both filters must be finalised");
    if (c->comm || c->comm_world > 1 || !c->local_group.empty())
        return fail(c, MG_ERR_STATE, "mg_cohort_begin: the context is part of a multi-GPU group (cohort mode and mg_comm_* do not combine)");
    if (reads_unfinished(c)) return fail(c, MG_ERR_STATE, "mg_cohort_begin: a reads count is open (mg_reads_finish first)");
    TRY(unjoin(c));
    BFState &b = c->bf[MG_BF_ALT];
    MapState &m = c->map;
    u32 shift = 0;
    while ((1u << shift) < n_planes) ++shift;
    const u64 nb = (b.nset ? b.nset : 1) << shift, nm = (m.vals_cap ? m.vals_cap : 1) << shift;
    u32 *pc = nullptr, *pv = nullptr;
    if (hipMalloc(&pc, nb * 4) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MG_ERR_NOMEM, "mg_cohort_begin: %u planes of %llu counters do not fit", n_planes, (unsigned long long)(b.nset + m.vals_cap));
    }
    if (hipMalloc(&pv, nm * 4) != hipSuccess) {
        hipFree(pc);
        (void)hipGetLastError(); // (the caller may go on with fewer planes: the runtime's sticky last-error must not surface in its next launch check)
        return fail(c, MG_ERR_NOMEM, "mg_cohort_begin: %u planes of %llu counters do not fit", n_planes, (unsigned long long)(b.nset + m.vals_cap));
    }
    hipError_t e = hipMemsetAsync(pc, 0, nb * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(pv, 0, nm * 4, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        hipFree(pc);
        hipFree(pv);
        return fail(c, MG_ERR_HIP, "mg_cohort_begin: clearing the planes: %s", hipGetErrorString(e));
    }
    c->coh_sv_counts = b.counts;
    c->coh_sv_vals = m.vals;
    b.counts = pc;
    m.vals = pv;
    c->coh_irr.assign(n_planes + 1, m.irregular);
    for (u32 s = 0; s < n_planes; ++s)
        for (auto &kv : c->coh_irr[s]) kv.second = 0;
    m.irregular = c->coh_irr[0];
    c->coh_planes = n_planes;
    c->coh_shift = shift;
    c->coh_sel = 0;
    c->rec_ok = false;
    c->vec_stale = c->vec_zero = false;
    return MG_OK;
}
MG_EXPORT int mg_cohort_select(mg_ctx *c, uint32_t plane)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->coh_planes) return fail(c, MG_ERR_STATE, "mg_cohort_select: not in cohort mode");
    if (plane >= c->coh_planes) return fail(c, MG_ERR_ARG, "mg_cohort_select: plane %u of %u", plane, c->coh_planes);
    if (reads_unfinished(c)) return fail(c, MG_ERR_STATE, "mg_cohort_select: a reads count is open (mg_reads_finish first)");
    if (plane != c->coh_sel) {
        c->coh_irr[c->coh_sel].swap(c->map.irregular);
        c->map.irregular.swap(c->coh_irr[plane]);
        c->coh_sel = plane;
    }
    return MG_OK;
}
MG_EXPORT int mg_cohort_end(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (!c) return MG_ERR_ARG;
    if (!c->coh_planes) return fail(c, MG_ERR_STATE, "mg_cohort_end: not in cohort mode");
    if (reads_unfinished(c)) return fail(c, MG_ERR_STATE, "mg_cohort_end: a reads count is open (mg_reads_finish first)");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    BFState &b = c->bf[MG_BF_ALT];
    MapState &m = c->map;
    hipFree(b.counts);
    hipFree(m.vals);
    b.counts = c->coh_sv_counts;
    m.vals = c->coh_sv_vals;
    c->coh_sv_counts = c->coh_sv_vals = nullptr;
    m.irregular.swap(c->coh_irr[c->coh_planes]);
    for (auto &kv : m.irregular) kv.second = 0;
    c->coh_irr.clear();
    c->coh_planes = c->coh_shift = c->coh_sel = 0;
    if (b.nset) HIP_TRY(c, hipMemsetAsync(b.counts, 0, b.nset * 4, c->stream));
    if (m.rows_total) HIP_TRY(c, hipMemsetAsync(m.vals, 0, m.rows_total * 4, c->stream));
    c->rec_ok = false; // the next single-sample scan republishes the records' copies from the (zero) vectors
    c->vec_stale = false;
    c->vec_zero = !c->rec_off;
    return MG_OK;
}
MG_EXPORT int mg_cohort_info(mg_ctx *c, uint32_t *n_planes, uint32_t *selected)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (n_planes) *n_planes = c->coh_planes;
    if (selected) *selected = c->coh_sel;
    return MG_OK;
}

// ---- multi-GPU exchange: RCCL over xGMI -----------------------------------------------------
// The scan shards by table rows; what has to be combined afterwards is one vector of wrapping u32 sums
// (mg_counters_view).  One ncclAllReduce(sum, uint32) over it, in place, on the context's stream.
// librccl is opened on first use: a single-GPU run never maps its half gigabyte, and a process that has already
// mapped a librccl.so.1 (PyTorch-ROCm bundles one) gets that copy -- one RCCL, like one HIP runtime, per process.
namespace {
struct Rccl {
    void *h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string err;
};
Rccl *rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (r.h) break;
        }
        if (!r.h) {
            const char *e = dlerror();
            r.err = std::string("cannot open librccl.so.1: ") + (e ? e : "?");
            return;
        }
        bool ok = true;
        auto sym = [&](const char *n) {
            void *p = dlsym(r.h, n);
            if (!p) {
                ok = false;
                r.err = std::string("librccl lacks ") + n;
            }
            return p;
        };
        r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
        r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
        r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
        r.AllReduce = (decltype(r.AllReduce))sym("ncclAllReduce");
        r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
        r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
        r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
        if (!ok) r.h = nullptr;
    });
    return r.h ? &r : nullptr;
}
#define NCCL_TRY(c, R, expr)                                                                           \
    do {                                                                                               \
        ncclResult_t r_ = (expr);                                                                      \
        if (r_ != ncclSuccess) return fail(c, MG_ERR_COMM, "%s: %s", #expr, (R)->GetErrorString(r_)); \
    } while (0)

// sum of up to MG_MAX_LOCAL counter vectors that live on ONE device, written back to all of them
constexpr int MG_MAX_LOCAL = 16;
struct LocalPtrs {
    u32 *p[MG_MAX_LOCAL];
    int n;
};
__global__ void __launch_bounds__(TPB) local_sum_kernel(LocalPtrs v, u64 n)
{
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TPB) {
        u32 s = 0;
        for (int j = 0; j < v.n; ++j) s += v.p[j][i];
        for (int j = 0; j < v.n; ++j) v.p[j][i] = s;
    }
}
// ---- the 16-bit packed form of the exchange --------------------------------------------------------------------------------
// Two counters travel in one 32-bit word (low and high half).  That is exact iff no half can carry into its neighbour, i.e.
// iff every rank's every partial counter is <= 65535 / world: checked first (a max over the vector, then over the ranks), the
// plain 32-bit sum runs otherwise.  Partial counters are small in practice: KMC lists each distinct k-mer once, so a counter
// receives one count (<= 255) plus those of the few k-mers that share it.  Half the bytes on the links.
__global__ void __launch_bounds__(TPB) vec_max_kernel(const u32 *__restrict__ v, u64 n, u32 *out)
{
    u32 m = 0;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TPB) m = max(m, v[i]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, (u32)__shfl_down((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
__global__ void __launch_bounds__(TPB) pack16_kernel(const u32 *__restrict__ v, u64 n, u32 *__restrict__ packed)
{
    const u64 m = n / 2;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < m + (n & 1); i += (u64)gridDim.x * TPB)
        packed[i] = i < m ? (v[2 * i] | v[2 * i + 1] << 16) : v[n - 1]; // (an odd last counter travels whole)
}
__global__ void __launch_bounds__(TPB) unpack16_kernel(u32 *__restrict__ v, u64 n, const u32 *__restrict__ packed)
{
    const u64 m = n / 2;
    for (u64 i = (u64)blockIdx.x * TPB + threadIdx.x; i < m + (n & 1); i += (u64)gridDim.x * TPB) {
        const u32 w = packed[i];
        if (i < m) {
            v[2 * i] = w & 0xFFFFu;
            v[2 * i + 1] = w >> 16;
        } else
            v[n - 1] = w;
    }
}
bool pack_wanted(const mg_ctx *c, u64 nn, int world)
{
    if (!c->exchange_pack || nn < 2 || world > 16) return false;
    return c->exchange_pack == 2 || nn * 4 >= (u64)c->exchange_pack_min_mb << 20;
}
// this context's largest counter -> *c->d_xmax (device), on stream `st`
int local_max(mg_ctx *c, u64 nn, hipStream_t st)
{
    if (!c->d_xmax) HIP_TRY(c, hipMalloc(&c->d_xmax, 8));
    HIP_TRY(c, hipMemsetAsync(c->d_xmax, 0, 4, st));
    hipLaunchKernelGGL(vec_max_kernel, dim3((unsigned)std::min<u64>(nblocks(nn), 2048u)), dim3(TPB), 0, st, (const u32 *)c->joined, nn, c->d_xmax);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int pack_into_scratch(mg_ctx *c, u64 nn, hipStream_t st, u32 **out)
{
    void *p;
    TRY(scratch(c, c->s_pack, (nn / 2 + 1) * 4, &p));
    hipLaunchKernelGGL(pack16_kernel, dim3((unsigned)std::min<u64>(nblocks(nn / 2 + 1), 4096u)), dim3(TPB), 0, st, (const u32 *)c->joined, nn, (u32 *)p);
    HIP_TRY(c, hipGetLastError());
    *out = (u32 *)p;
    return MG_OK;
}
int comm_drop(mg_ctx *c)
{
    if (c->comm) {
        Rccl *R = rccl();
        if (R) R->CommDestroy(c->comm);
        c->comm = nullptr;
    }
    for (mg_ctx *o : c->local_group) // a local group dissolves as a whole
        if (o != c) o->local_group.clear();
    c->local_group.clear();
    c->comm_world = 0;
    c->comm_rank = 0;
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_comm_unique_id(void *id_out)
{
    if (!id_out) return MG_ERR_ARG;
    Rccl *R = rccl();
    if (!R) return MG_ERR_COMM;
    static_assert(sizeof(ncclUniqueId) == MG_COMM_ID_BYTES, "MG_COMM_ID_BYTES");
    ncclUniqueId id;
    if (R->GetUniqueId(&id) != ncclSuccess) return MG_ERR_COMM;
    memcpy(id_out, &id, sizeof id);
    return MG_OK;
}

MG_EXPORT int mg_comm_init(mg_ctx *c, int rank, int world, const void *id)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (world < 1 || rank < 0 || rank >= world || !id) return fail(c, MG_ERR_ARG, "mg_comm_init: rank %d of %d", rank, world);
    Rccl *R = rccl();
    if (!R) return fail(c, MG_ERR_COMM, "RCCL unavailable");
    comm_drop(c);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    NCCL_TRY(c, R, R->CommInitRank(&c->comm, world, uid, rank));
    c->comm_rank = rank;
    c->comm_world = world;
    return MG_OK;
}

MG_EXPORT int mg_comm_init_all(mg_ctx **ctxs, int n)
{
    if (!ctxs || n < 1 || n > 64) return MG_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return MG_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (ctxs[i]->coh_planes) return fail(ctxs[i], MG_ERR_STATE, "mg_comm_init_all: context %d is in cohort mode (mg_cohort_end first)", i);
    bool distinct = true, same = true;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) {
            if (ctxs[i] == ctxs[j]) return fail(ctxs[0], MG_ERR_ARG, "mg_comm_init_all: context %d listed twice", i);
            if (ctxs[i]->device == ctxs[j]->device) distinct = false;
            else same = false;
        }
    for (int i = 0; i < n; ++i) comm_drop(ctxs[i]);
    if (n == 1 || distinct) { // one rank per device: RCCL (n == 1 too, so that a single-GPU run drives the same calls)
        Rccl *R = rccl();
        if (!R) return fail(ctxs[0], MG_ERR_COMM, "RCCL unavailable");
        ncclUniqueId uid;
        NCCL_TRY(ctxs[0], R, R->GetUniqueId(&uid));
        int prev = -1;
        hipGetDevice(&prev);
        NCCL_TRY(ctxs[0], R, R->GroupStart());
        ncclResult_t bad = ncclSuccess;
        for (int i = 0; i < n && bad == ncclSuccess; ++i) {
            hipSetDevice(ctxs[i]->device);
            bad = R->CommInitRank(&ctxs[i]->comm, n, uid, i);
        }
        const ncclResult_t ge = R->GroupEnd();
        if (prev >= 0) hipSetDevice(prev);
        if (bad != ncclSuccess || ge != ncclSuccess) {
            for (int i = 0; i < n; ++i) { // communicators the group did create are destroyed, not dropped
                if (ctxs[i]->comm) R->CommDestroy(ctxs[i]->comm);
                ctxs[i]->comm = nullptr;
            }
            return fail(ctxs[0], MG_ERR_COMM, "ncclCommInitRank x%d: %s", n, R->GetErrorString(bad != ncclSuccess ? bad : ge));
        }
        for (int i = 0; i < n; ++i) {
            ctxs[i]->comm_rank = i;
            ctxs[i]->comm_world = n;
        }
        return MG_OK;
    }
    if (!same) return fail(ctxs[0], MG_ERR_ARG, "mg_comm_init_all: contexts must sit on distinct devices, or all on one");
    if (n > MG_MAX_LOCAL) return fail(ctxs[0], MG_ERR_LIMIT, "at most %d contexts may share a device", MG_MAX_LOCAL);
    // all on one device (a rehearsal of the N-GPU layout on a one-GPU box: RCCL rejects duplicate devices)
    for (int i = 0; i < n; ++i) {
        ctxs[i]->local_group.assign(ctxs, ctxs + n);
        ctxs[i]->comm_rank = i;
        ctxs[i]->comm_world = n;
        if (!ctxs[i]->ev_x) {
            const DeviceGuard g(ctxs[i]);
            if (hipEventCreateWithFlags(&ctxs[i]->ev_x, hipEventDisableTiming) != hipSuccess) return fail(ctxs[i], MG_ERR_HIP, "hipEventCreate");
        }
    }
    return MG_OK;
}

MG_EXPORT int mg_comm_destroy(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (!c) return MG_ERR_ARG;
    return comm_drop(c);
}

MG_EXPORT int mg_comm_info(mg_ctx *c, int *rank, int *world, int *backend)
{
    if (!c) return MG_ERR_ARG;
    if (rank) *rank = c->comm_rank;
    if (world) *world = c->comm_world;
    if (backend) *backend = c->comm ? MG_COMM_RCCL : !c->local_group.empty() ? MG_COMM_LOCAL : MG_COMM_NONE;
    return MG_OK;
}

namespace {
// The exchange of one context's counters over its RCCL communicator, enqueued on `st`.  With the packed form the call waits
// (the host has to see the ranks' largest partial counter to choose the form; every rank sees the same one).
int exchange_rccl(mg_ctx *c, hipStream_t st)
{
    Rccl *R = rccl();
    const u64 nn = c->bf[MG_BF_ALT].nset + c->map.rows_total;
    c->last_exchange_packed = 0;
    if (nn == 0) return MG_OK;
    bool packed = false;
    if (pack_wanted(c, nn, c->comm_world)) {
        TRY(local_max(c, nn, st));
        NCCL_TRY(c, R, R->AllReduce(c->d_xmax, c->d_xmax, 1, ncclUint32, ncclMax, c->comm, st));
        u32 mx = 0;
        HIP_TRY(c, hipMemcpyAsync(&mx, c->d_xmax, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        packed = mx <= 65535u / (u32)c->comm_world;
    }
    if (c->x_timed) HIP_TRY(c, hipEventRecord(c->ev_xs[2], st));
    if (packed) {
        u32 *pk;
        TRY(pack_into_scratch(c, nn, st, &pk));
        NCCL_TRY(c, R, R->AllReduce(pk, pk, nn / 2 + (nn & 1), ncclUint32, ncclSum, c->comm, st));
        hipLaunchKernelGGL(unpack16_kernel, dim3((unsigned)std::min<u64>(nblocks(nn / 2 + 1), 4096u)), dim3(TPB), 0, st, c->joined, nn, (const u32 *)pk);
        HIP_TRY(c, hipGetLastError());
    } else
        NCCL_TRY(c, R, R->AllReduce(c->joined, c->joined, nn, ncclUint32, ncclSum, c->comm, st));
    if (c->x_timed) HIP_TRY(c, hipEventRecord(c->ev_xs[3], st));
    c->last_exchange_packed = packed ? 1 : 0;
    return MG_OK;
}
int exchange_ready(mg_ctx *c)
{
    if (!c->comm) return fail(c, MG_ERR_STATE, "no RCCL communicator (mg_comm_init first; contexts sharing a device use mg_counters_allreduce_all)");
    TRY(ensure_joined(c));
    for (int i = 0; i < 4; ++i)
        if (!c->ev_xs[i]) HIP_TRY(c, i < 2 ? hipEventCreateWithFlags(&c->ev_xs[i], hipEventDisableTiming) : hipEventCreate(&c->ev_xs[i]));
    c->x_timed = true;
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_counters_allreduce(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    TRY(exchange_ready(c));
    return exchange_rccl(c, c->stream);
}
// The same exchange on a stream of its own: _begin orders it behind everything the context's stream holds so far (the scan),
// _end makes the context's stream wait for it.  In between the caller may enqueue what needs no counters -- the block cut of the
// record loop (mg_cut_blocks_device) -- which then runs beside the collective instead of behind it.
MG_EXPORT int mg_counters_allreduce_begin(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (c->x_pending) return fail(c, MG_ERR_STATE, "mg_counters_allreduce_begin twice without mg_counters_allreduce_end");
    TRY(exchange_ready(c));
    if (!c->xstream) HIP_TRY(c, hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventRecord(c->ev_xs[0], c->stream));
    HIP_TRY(c, hipStreamWaitEvent(c->xstream, c->ev_xs[0], 0));
    TRY(exchange_rccl(c, c->xstream));
    HIP_TRY(c, hipEventRecord(c->ev_xs[1], c->xstream));
    c->x_pending = true;
    return MG_OK;
}
MG_EXPORT int mg_counters_allreduce_end(mg_ctx *c)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (!c->x_pending) return fail(c, MG_ERR_STATE, "mg_counters_allreduce_end without mg_counters_allreduce_begin");
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_xs[1], 0));
    c->x_pending = false;
    return MG_OK;
}
// duration of the most recent exchange of this context (its collective with pack / unpack, without the guard's max), and its form
MG_EXPORT int mg_exchange_stats(mg_ctx *c, float *ms_out, int *packed_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->x_timed || !c->ev_xs[3]) return fail(c, MG_ERR_STATE, "no exchange has run");
    HIP_TRY(c, hipEventSynchronize(c->ev_xs[3]));
    if (ms_out) HIP_TRY(c, hipEventElapsedTime(ms_out, c->ev_xs[2], c->ev_xs[3]));
    if (packed_out) *packed_out = c->last_exchange_packed;
    return MG_OK;
}

MG_EXPORT int mg_counters_allreduce_all(mg_ctx **ctxs, int n)
{
    if (!ctxs || n < 1) return MG_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return MG_ERR_ARG;
    mg_ctx *c0 = ctxs[0];
    u64 nn = 0;
    for (int i = 0; i < n; ++i)
        if (ctxs[i]->coh_planes) return fail(ctxs[i], MG_ERR_STATE, "mg_counters_allreduce_all: context %d is in cohort mode (mg_cohort_end first)", i);
    for (int i = 0; i < n; ++i) {
        const DeviceGuard g(ctxs[i]);
        TRY(ensure_joined(ctxs[i]));
        const u64 ni = ctxs[i]->bf[MG_BF_ALT].nset + ctxs[i]->map.rows_total;
        if (i && (ni != nn || ctxs[i]->bf[MG_BF_ALT].nset != c0->bf[MG_BF_ALT].nset))
            return fail(c0, MG_ERR_STATE, "context %d holds another index (%llu counters, context 0 %llu): every rank must load the same index",
                        i, (unsigned long long)ni, (unsigned long long)nn);
        nn = ni;
        if (ctxs[i]->comm_world != n) return fail(c0, MG_ERR_STATE, "context %d is not part of a %d-way group (mg_comm_init_all)", i, n);
        ctxs[i]->last_exchange_packed = 0;
    }
    if (nn == 0) return MG_OK;
    // the packed form's guard: every context's largest partial counter, seen by this one process (no collective needed)
    bool packed = false;
    if (pack_wanted(c0, nn, n)) {
        u32 mx = 0;
        for (int i = 0; i < n; ++i) {
            const DeviceGuard g(ctxs[i]);
            TRY(local_max(ctxs[i], nn, ctxs[i]->stream));
        }
        for (int i = 0; i < n; ++i) {
            const DeviceGuard g(ctxs[i]);
            u32 m1 = 0;
            HIP_TRY(ctxs[i], hipMemcpyAsync(&m1, ctxs[i]->d_xmax, 4, hipMemcpyDeviceToHost, ctxs[i]->stream));
            HIP_TRY(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));
            mx = std::max(mx, m1);
        }
        packed = mx <= 65535u / (u32)n;
    }
    const u64 np = nn / 2 + (nn & 1);
    if (c0->comm) { // one rank per device, one process: a group of all-reduces, each on its context's stream
        Rccl *R = rccl();
        int prev = -1;
        hipGetDevice(&prev);
        std::vector<u32 *> pk((size_t)n, nullptr);
        if (packed)
            for (int i = 0; i < n; ++i) {
                hipSetDevice(ctxs[i]->device);
                TRY(pack_into_scratch(ctxs[i], nn, ctxs[i]->stream, &pk[(size_t)i]));
            }
        NCCL_TRY(c0, R, R->GroupStart());
        ncclResult_t bad = ncclSuccess;
        for (int i = 0; i < n && bad == ncclSuccess; ++i) {
            hipSetDevice(ctxs[i]->device);
            bad = packed ? R->AllReduce(pk[(size_t)i], pk[(size_t)i], np, ncclUint32, ncclSum, ctxs[i]->comm, ctxs[i]->stream)
                         : R->AllReduce(ctxs[i]->joined, ctxs[i]->joined, nn, ncclUint32, ncclSum, ctxs[i]->comm, ctxs[i]->stream);
        }
        const ncclResult_t ge = R->GroupEnd();
        if (packed && bad == ncclSuccess && ge == ncclSuccess)
            for (int i = 0; i < n; ++i) {
                hipSetDevice(ctxs[i]->device);
                hipLaunchKernelGGL(unpack16_kernel, dim3((unsigned)std::min<u64>(nblocks(np), 4096u)), dim3(TPB), 0, ctxs[i]->stream, ctxs[i]->joined, nn, (const u32 *)pk[(size_t)i]);
                ctxs[i]->last_exchange_packed = 1;
            }
        if (prev >= 0) hipSetDevice(prev);
        if (bad != ncclSuccess || ge != ncclSuccess) return fail(c0, MG_ERR_COMM, "ncclAllReduce x%d: %s", n, R->GetErrorString(bad != ncclSuccess ? bad : ge));
        return MG_OK;
    }
    if (c0->local_group.size() != (size_t)n) return fail(c0, MG_ERR_STATE, "mg_comm_init_all first");
    // contexts sharing one device: context 0's stream waits for every scan, sums (the packed words, where that form applies:
    // the same pack / unpack kernels as on the wire), and everyone waits for the sum
    const DeviceGuard g(c0);
    LocalPtrs v{};
    v.n = n;
    for (int i = 0; i < n; ++i) {
        if (i) {
            HIP_TRY(c0, hipEventRecord(ctxs[i]->ev_x, ctxs[i]->stream));
            HIP_TRY(c0, hipStreamWaitEvent(c0->stream, ctxs[i]->ev_x, 0));
        }
        if (packed) TRY(pack_into_scratch(ctxs[i], nn, c0->stream, &v.p[i]));
        else v.p[i] = ctxs[i]->joined;
    }
    hipLaunchKernelGGL(local_sum_kernel, dim3((unsigned)std::min<u64>(nblocks(packed ? np : nn), 4096u)), dim3(TPB), 0, c0->stream, v, packed ? np : nn);
    HIP_TRY(c0, hipGetLastError());
    if (packed)
        for (int i = 0; i < n; ++i) {
            hipLaunchKernelGGL(unpack16_kernel, dim3((unsigned)std::min<u64>(nblocks(np), 4096u)), dim3(TPB), 0, c0->stream, ctxs[i]->joined, nn, (const u32 *)v.p[i]);
            ctxs[i]->last_exchange_packed = 1;
        }
    HIP_TRY(c0, hipGetLastError());
    HIP_TRY(c0, hipEventRecord(c0->ev_x, c0->stream));
    for (int i = 1; i < n; ++i) HIP_TRY(c0, hipStreamWaitEvent(ctxs[i]->stream, c0->ev_x, 0));
    return MG_OK;
}

// ---- per-variant path -----------------------------------------------------------------------

MG_EXPORT int mg_lookup_cover(mg_ctx *c, const char *rows, size_t stride, size_t n_rows, const uint8_t *is_ref,
                              const uint64_t *sig_kmer_off, size_t n_sigs, const uint64_t *allele_sig_off, size_t n_alleles,
                              uint32_t *cov_out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_rows(c, rows, stride, n_rows));
    if (n_alleles == 0) return MG_OK;
    if (!sig_kmer_off || !allele_sig_off || !cov_out || (n_rows && !is_ref)) return fail(c, MG_ERR_ARG, "NULL descriptor");
    if (allele_sig_off[n_alleles] != n_sigs || sig_kmer_off[n_sigs] != n_rows)
        return fail(c, MG_ERR_ARG, "descriptor offsets do not close (sigs %zu rows %zu)", n_sigs, n_rows);
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    void *d_rows, *d_isref, *d_w, *d_so, *d_ao, *d_cov;
    TRY(upload(c, c->s_rows, rows, stride * n_rows, &d_rows));
    TRY(upload(c, c->s_misc[0], is_ref, n_rows, &d_isref));
    TRY(scratch(c, c->s_out, 4 * (n_rows ? n_rows : 1), &d_w));
    TRY(upload(c, c->s_misc[2], sig_kmer_off, 8 * (n_sigs + 1), &d_so));
    TRY(upload(c, c->s_misc[3], allele_sig_off, 8 * (n_alleles + 1), &d_ao));
    TRY(scratch(c, c->s_misc[4], 4 * n_alleles, &d_cov));
    if (n_rows) {
        // exact-map keys the packed table cannot hold (every key, when k > MG_MAX_PACKED_K) live in the context's host list:
        // the kernel marks such rows and their values are filled in from there (KMAP::get_count, kmap.hpp:124-131)
        void *d_irr = nullptr;
        const bool host_keys = !c->map.irregular.empty();
        if (host_keys) {
            TRY(scratch(c, c->s_irr, n_rows, &d_irr));
            HIP_TRY(c, hipMemsetAsync(d_irr, 0, n_rows, c->stream));
        }
        hipLaunchKernelGGL(rows_kernel<OP_WEIGHT>, dim3(nblocks(n_rows)), dim3(TPB), 0, c->stream, (const u8 *)d_rows, stride,
                           n_rows, view(c, MG_BF_ALT), view(c), (const u32 *)nullptr, (const u8 *)d_isref, d_w,
                           (u8 *)d_irr);
        HIP_TRY(c, hipGetLastError());
        if (host_keys) {
            std::vector<u8> irr(n_rows);
            std::vector<i32> w(n_rows);
            HIP_TRY(c, hipMemcpyAsync(irr.data(), d_irr, n_rows, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(w.data(), d_w, 4 * n_rows, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            bool any = false;
            for (size_t i = 0; i < n_rows; ++i)
                if (irr[i]) {
                    auto it = c->map.irregular.find(host_irregular_key(rows + i * stride, stride));
                    w[i] = it != c->map.irregular.end() ? it->second : 0;
                    any = true;
                }
            if (any) {
                HIP_TRY(c, hipMemcpyAsync(d_w, w.data(), 4 * n_rows, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream)); // (w leaves scope)
            }
        }
    }
    hipLaunchKernelGGL(cover_kernel, dim3(nblocks(n_alleles)), dim3(TPB), 0, c->stream, (const i32 *)d_w, (const u64 *)d_so,
                       (const u64 *)d_ao, (u64)n_alleles, (u32 *)d_cov);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cov_out, d_cov, 4 * n_alleles, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_genotype_device(mg_ctx *c, const void *d_cov, const void *d_freq, const void *d_var_allele_off, size_t n_vars, float error_rate,
                                 int max_cov, int haploid, void *d_gt1, void *d_gt2, void *d_gq, void *d_status, void *d_probs, const void *d_var_gt_off)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (n_vars == 0) return MG_OK;
    if (!d_cov || !d_freq || !d_var_allele_off || !d_gt1 || !d_gt2 || !d_gq || !d_status) return fail(c, MG_ERR_ARG, "NULL argument");
    if (d_probs && !d_var_gt_off) return fail(c, MG_ERR_ARG, "probs needs var_gt_off");
    GenoParams p;
    TRY(fill_geno_params(c, error_rate, max_cov, haploid, &p));
    hipLaunchKernelGGL(genotype_kernel, dim3(nblocks(n_vars)), dim3(TPB), 0, c->stream, (const u32 *)d_cov, (const float *)d_freq,
                       (const u32 *)d_var_allele_off, (u64)n_vars, p, (i32 *)d_gt1, (i32 *)d_gt2, (i32 *)d_gq, (u8 *)d_status, (double *)d_probs,
                       (const u64 *)d_var_gt_off);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}

MG_EXPORT int mg_genotype(mg_ctx *c, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off, size_t n_vars,
                          float error_rate, int max_cov, int haploid, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status,
                          double *probs, const uint64_t *var_gt_off)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_vars == 0) return MG_OK;
    if (!cov || !freq || !var_allele_off || !gt1 || !gt2 || !gq || !status) return fail(c, MG_ERR_ARG, "NULL argument");
    if (probs && !var_gt_off) return fail(c, MG_ERR_ARG, "probs needs var_gt_off");
    const size_t na = var_allele_off[n_vars];
    const size_t ng = probs ? var_gt_off[n_vars] : 0;
    void *d_cov, *d_freq, *d_off, *d_g1, *d_g2, *d_gq, *d_st, *d_pr = nullptr, *d_go = nullptr;
    TRY(upload(c, c->s_rows, cov, 4 * na, &d_cov));
    TRY(upload(c, c->s_aux, freq, 4 * na, &d_freq));
    TRY(upload(c, c->s_misc[0], var_allele_off, 4 * (n_vars + 1), &d_off));
    TRY(scratch(c, c->s_misc[1], 4 * n_vars, &d_g1));
    TRY(scratch(c, c->s_misc[2], 4 * n_vars, &d_g2));
    TRY(scratch(c, c->s_misc[3], 4 * n_vars, &d_gq));
    TRY(scratch(c, c->s_misc[4], n_vars, &d_st));
    if (probs) {
        TRY(scratch(c, c->s_out, 8 * (ng ? ng : 1), &d_pr));
        TRY(upload(c, c->s_misc[5], var_gt_off, 8 * (n_vars + 1), &d_go));
    }
    TRY(mg_genotype_device(c, d_cov, d_freq, d_off, n_vars, error_rate, max_cov, haploid, d_g1, d_g2, d_gq, d_st, d_pr, d_go));
    HIP_TRY(c, hipMemcpyAsync(gt1, d_g1, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gt2, d_g2, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gq, d_gq, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, d_st, n_vars, hipMemcpyDeviceToHost, c->stream));
    if (probs && ng) HIP_TRY(c, hipMemcpyAsync(probs, d_pr, 8 * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // records that took an ln(n) from the device's log(double): again on the host, with libm (host_genotype_one)
    for (size_t v = 0; v < n_vars; ++v) {
        if (status[v] != 0) continue;
        const uint32_t a0 = var_allele_off[v], A = var_allele_off[v + 1] - a0;
        int isum = 0;
        for (uint32_t a = 0; a < A; ++a) isum += (int)cov[a0 + a];
        if (isum < MG_LN_TABLE) continue;
        host_genotype_one(cov + a0, freq + a0, (int)A, (u32)isum, error_rate, haploid, gt1 + v, gt2 + v, gq + v, probs ? probs + var_gt_off[v] : nullptr);
    }
    return MG_OK;
}

namespace {
// ---- blocks on the device ------------------------------------------------------------------------------------------------
// flags (one byte per record, set at the first record of every block) -> blk_var_off / var_block / the block count:
// per-tile counts are already in `tile_sums` (cut_flags_kernel / flag_count_kernel wrote them)
int scan_flags(mg_ctx *c, u64 n, const u8 *d_flags, u32 *d_tile_sums, u32 *d_blk_var_off, u32 *d_var_block, unsigned long long *d_n_blocks)
{
    const u64 n_tiles = nblocks(n);
    TRY(launch_tile_scan(c, d_tile_sums, n_tiles, c->d_hit_count + 2)); // (the total is re-derived by the scatter)
    hipLaunchKernelGGL(flag_scatter_kernel, dim3((unsigned)n_tiles), dim3(TPB), 0, c->stream, n, d_flags, (const u32 *)d_tile_sums, d_blk_var_off, d_var_block,
                       d_n_blocks);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int check_panel(mg_ctx *c, const mg_panel_dev *p, bool need_gt)
{
    if (!p) return fail(c, MG_ERR_ARG, "NULL panel");
    if (p->n_vars >= 0xFFFFFFFFull) return fail(c, MG_ERR_LIMIT, "fewer than 2^32 records per batch");
    if (p->n_vars == 0) return MG_OK;
    if (!p->contig_id || !p->pos || !p->ref_size || !p->min_size) return fail(c, MG_ERR_ARG, "NULL panel array");
    if (need_gt && (!p->contig_base || !p->contig_len || !p->present || !p->var_allele_off || !p->allele_off || !p->pool || !p->canon ||
                    (p->n_samples && !p->gt && !p->sp_off) || (p->sp_off && (!p->sp_sample || !p->sp_gt))))
        return fail(c, MG_ERR_ARG, "NULL panel array");
    return MG_OK;
}
PanelView panel_view(const mg_panel_dev *p)
{
    PanelView P{};
    P.contig_base = p->contig_base; P.contig_len = p->contig_len; P.contig_id = p->contig_id; P.pos = p->pos;
    P.ref_size = p->ref_size; P.min_size = p->min_size; P.present = p->present; P.var_allele_off = p->var_allele_off;
    P.allele_off = p->allele_off; P.canon = p->canon; P.gt = p->gt; P.n_samples = p->n_samples;
    P.sp_off = p->sp_off; P.sp_sample = p->sp_sample; P.sp_gt = p->sp_gt; P.sp_default = p->sp_default;
    return P;
}
// The tiers of block_pipeline.h over one resident panel.  Counts stay on the device; c->d_gen_count holds
//   [0] general records listed by tier 1   [1] insertion-row cursor (index time) / block count of a host-form batch
//   [2] signature k-mers of the lone records   [3] signature k-mers tiers 2 and 3 assembled   [4] records tier 3 took
struct BlocksRun {
    mg_ctx *c;
    const mg_panel_dev *p;
    BlockBatch B;
    PanelView P;
    u32 *gen_list, *fb_list;
    u8 *fb_flag;
    CombDesc *combs;
    PickItem *items, *slides;
    u32 *retry, *order;
    unsigned long long *round_counters;
    u64 round, n_rounds;
    int cus;
};
int blocks_setup(mg_ctx *c, const mg_panel_dev *p, const u32 *d_blk_var_off, const u32 *d_var_block, const unsigned long long *d_n_blocks, int haploid, BlocksRun *out)
{
    const u64 n = p->n_vars;
    if (!c->d_ref) return fail(c, MG_ERR_STATE, "mg_reference_upload first");
    BlocksRun R{};
    R.c = c;
    R.p = p;
    // general records per round of tier 2.  The list's length lives on the device, so ceil(n / round) rounds are launched and those
    // beyond its end find nothing to do -- at ~30 us of empty launches each: 2^24 records per round (13.5 GB of round buffers at most,
    // of 288) leaves a whole-genome panel 5 rounds instead of 20
    R.round = std::min<u64>(n, 1ULL << c->blocks_round_log2);
    R.n_rounds = (n + R.round - 1) / R.round;
    void *q[8];
    TRY(scratch(c, c->s_blk[0], 4 * n, &q[0]));                                                   // gen_list
    TRY(scratch(c, c->s_blk[1], 4 * n, &q[1]));                                                   // fb_list
    TRY(scratch(c, c->s_blk[2], n, &q[2]));                                                       // fb_flag
    TRY(scratch(c, c->s_blk[3], sizeof(CombDesc) * (R.round * FW_COMBS_PER_REC + 64), &q[3]));    // one round's descriptors
    TRY(scratch(c, c->s_blk[4], sizeof(PickItem) * (R.round * FW_ITEMS_PER_REC + FW_CHUNK * (u64)(1 << 14)), &q[4])); // one round's items (+ a chunk per wave)
    TRY(scratch(c, c->s_blk[5], 8 * FW_ROUND_COUNTERS * R.n_rounds, &q[5]));                      // per round: descriptors, items, sliding items reserved, chains per length
    TRY(scratch(c, c->s_blk[6], sizeof(PickItem) * (R.round / 4 + 4096), &q[7]));                 // one round's sliding items
    void *q_retry, *q_order;
    TRY(scratch(c, c->s_blk[7], 4 * (R.round * FW_COMBS_PER_REC + 64), &q_retry));                // one round's chains to retry
    TRY(scratch(c, c->s_blk[13], 4 * (R.round * FW_COMBS_PER_REC + 64), &q_order));               // one round's chains in order of their length
    void *q_class;
    TRY(scratch(c, c->s_blk[14], 2 * n, &q_class));                                               // per listed record: REC_* and the alleles' codes
    if (!d_var_block) { // derive it from the cut: heads -> scan
        void *fl, *ts;
        TRY(scratch(c, c->s_blk[8], 4 * n, &q[6]));
        TRY(scratch(c, c->s_blk[9], n, &fl));
        TRY(scratch(c, c->s_blk[10], 4 * (u64)nblocks(n) + 4, &ts));
        HIP_TRY(c, hipMemsetAsync(fl, 0, n, c->stream));
        hipLaunchKernelGGL(block_heads_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, d_blk_var_off, d_n_blocks, n, (u8 *)fl);
        hipLaunchKernelGGL(flag_count_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, n, (const u8 *)fl, (u32 *)ts);
        TRY(scan_flags(c, n, (const u8 *)fl, (u32 *)ts, nullptr, (u32 *)q[6], nullptr));
        d_var_block = (const u32 *)q[6];
    }
    if (!c->d_gen_count) HIP_TRY(c, hipMalloc(&c->d_gen_count, 64));
    BlockBatch B{};
    B.reference = c->d_ref;
    B.ref2 = c->d_ref2;
    B.refbad = c->d_refbad;
    B.contig_base = p->contig_base; B.contig_len = p->contig_len; B.contig_id = p->contig_id;
    B.blk_var_off = d_blk_var_off; B.var_block = d_var_block;
    B.pos = p->pos; B.ref_size = p->ref_size; B.min_size = p->min_size; B.present = p->present; B.var_allele_off = p->var_allele_off;
    B.allele_off = p->allele_off; B.pool = (const u8 *)p->pool; B.canon = p->canon; B.gt = p->gt;
    B.sp_off = p->sp_off; B.sp_sample = p->sp_sample; B.sp_gt = p->sp_gt; B.sp_default = p->sp_default;
    B.n_samples = p->n_samples; B.haploid = haploid; B.k = (int)c->k;
    B.set_limit = c->blocks_set_limit;
    B.snp_chains = c->use_snp_chains;
    B.rec_class = (const unsigned short *)q_class;
    // the alleles packed like the reference (every call: the panel is the caller's) -- unless the pool is too small to hold alleles worth
    // it (a SNP panel: two one-base alleles per record; fw_eval takes alleles of up to 4 bases from the bytes anyway)
    if (p->pool_bytes && p->pool_bytes * 2 > n * 5 && ((uintptr_t)p->pool & 3) == 0 && c->use_packed_pool) {
        void *p2, *pb;
        const u64 n_words = (p->pool_bytes + 31) / 32 + 4;
        TRY(scratch(c, c->s_blk[11], 8 * n_words, &p2));
        TRY(scratch(c, c->s_blk[12], 4 * n_words, &pb));
        TRY(reference_pack(c, (const u8 *)p->pool, p->pool_bytes, (u64 *)p2, (u32 *)pb));
        B.pool2 = (const u64 *)p2;
        B.poolbad = (const u32 *)pb;
    }
    R.B = B;
    R.P = panel_view(p);
    R.gen_list = (u32 *)q[0]; R.fb_list = (u32 *)q[1]; R.fb_flag = (u8 *)q[2];
    R.combs = (CombDesc *)q[3]; R.items = (PickItem *)q[4]; R.round_counters = (unsigned long long *)q[5];
    R.slides = (PickItem *)q[7];
    R.retry = (u32 *)q_retry;
    R.order = (u32 *)q_order;
    R.cus = device_cus(c);
    *out = R;
    return MG_OK;
}
// Tiles a workgroup of tier 1 takes, for `threads` threads in all (two a record; one at index time): as many as still leave the grid
// five eighths of the workgroups that are resident together (eight a CU) -- the kernel waits for random lines, and a smaller grid
// leaves wave slots empty while every thread walks its tiles one after the other; a larger one pays a reservation and two barriers
// per workgroup for nothing.  1e6 records on 256 CUs (7,813 tiles, 2,048 resident): 0.137 / 0.113 / 0.102 / 0.132 ms with 1 / 2 / 4 / 8
// tiles, so four (1,954 workgroups: all resident at once, no second round); 7e5: 0.086 / 0.082 / 0.109 with 2 / 4 / 8 (1,368 workgroups
// at four); 1.5e6: 0.157 / 0.159 / 0.155 (1,465 at eight).  The 977 workgroups of 1e6 records at eight are too few, 1,368 are enough.
// A whole-genome panel keeps LONE_TILES.
constexpr int LONE_WGS_PER_CU = 5;
int lone_tiles_for(mg_ctx *c, u64 threads)
{
    if (c->lone_tiles) return c->lone_tiles;
    const u64 n_tiles = (threads + TPB - 1) / TPB, want = (u64)device_cus(c) * LONE_WGS_PER_CU;
    int tiles = LONE_TILES;
    while (tiles > 1 && (n_tiles + tiles - 1) / tiles < want) tiles /= 2;
    return tiles;
}
unsigned lone_grid(u64 threads, int tiles) { return (unsigned)((threads + (u64)tiles * TPB - 1) / ((u64)tiles * TPB)); }
// the SLOW redo of tier 1: no more workgroups than the fast launch has, and no more than are worth starting to find nothing to do
unsigned lone_slow_grid(mg_ctx *c, unsigned fast_grid) { return std::min<unsigned>(fast_grid, (unsigned)device_cus(c) * 4); }
// what a cover call zeroes before tier 1 (blocks_clear_kernel): the records' flags, the call's counts or some of them, the rounds' counters
int blocks_clear(BlocksRun &R, u8 *d_overflow, unsigned long long *counts, u64 n_counts)
{
    mg_ctx *c = R.c;
    ClearJob J{};
    J.bytes[0] = d_overflow;
    J.bytes[1] = R.fb_flag;
    J.n = R.p->n_vars;
    J.words[0] = counts;
    J.n_words[0] = n_counts;
    J.words[1] = R.round_counters;
    J.n_words[1] = FW_ROUND_COUNTERS * R.n_rounds;
    const u64 units = std::max<u64>(J.n / 16 + 2, J.n_words[1]);
    hipLaunchKernelGGL(blocks_clear_kernel, dim3((unsigned)std::min<u64>(nblocks(units), (u64)R.cus * 8)), dim3(TPB), 0, c->stream, J);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
// tier 2 over the whole general list, round by round; the caller has zeroed the rounds' counters (blocks_clear, or a fill of its own)
template <int MODE> int blocks_tier2(BlocksRun &R, u32 *d_cov, u8 *d_overflow, unsigned long long *d_cursor, u32 row0, unsigned long long *d_evaluated)
{
    mg_ctx *c = R.c;
    if (c->use_flat_tier == 0) { // A/B and tests: everything general goes to the workgroup kernel
        hipLaunchKernelGGL(flag_all_kernel, dim3(R.cus * 8), dim3(TPB), 0, c->stream, (const u32 *)R.gen_list, (const unsigned long long *)c->d_gen_count, R.fb_flag,
                           MODE == 0 ? d_cov : (u32 *)nullptr, R.B.var_allele_off);
        HIP_TRY(c, hipGetLastError());
        return MG_OK;
    }
    c->last_rounds = R.n_rounds;
    for (u64 r = 0; r < R.n_rounds; ++r) {
        FlatWork W{};
        W.gen_list = R.gen_list;
        W.gen_count = c->d_gen_count;
        W.base = r * R.round;
        W.round_len = R.round;
        W.combs = R.combs;
        W.comb_cap = (u32)(R.round * FW_COMBS_PER_REC);
        W.items = R.items;
        W.item_cap = (u32)(R.round * FW_ITEMS_PER_REC + FW_CHUNK * (u64)(1 << 14));
        W.slides = R.slides;
        W.slide_cap = (u32)(R.round / 4 + 4096);
        W.retry = R.retry;
        W.counters = R.round_counters + FW_ROUND_COUNTERS * r;
        W.order = c->use_chain_order ? R.order : nullptr;
        W.fb_flag = R.fb_flag;
        hipLaunchKernelGGL(fw_walk_kernel<MODE>, dim3(nblocks(R.round)), dim3(TPB), 0, c->stream, R.B, W, d_cov, d_overflow);
        const u32 n_haps = R.B.haploid ? R.B.n_samples : 2 * R.B.n_samples;
        if (c->use_snp_kernel && R.B.snp_chains && n_haps <= FW_SNP_MAX_HAPS) { // chains of SNPs whole, before the picks kernel sees them
            int GH = 2;
            while ((u32)GH < n_haps) GH *= 2;
            hipLaunchKernelGGL(fw_snp_kernel<MODE>, dim3(R.cus * 8), dim3(TPB), 0, c->stream, R.B, W, GH, view(c, MG_BF_ALT), view(c), d_cov, d_cursor, row0, d_evaluated);
        }
        if (W.order) { // what is left, by length (grids sized for the round's worst case: workgroups beyond the chains written find nothing)
            const unsigned og = (unsigned)std::min<u64>(nblocks((u64)W.comb_cap), (u64)R.cus * 4);
            hipLaunchKernelGGL(fw_order_kernel<0>, dim3(og), dim3(TPB), 0, c->stream, W);
            hipLaunchKernelGGL(fw_order_kernel<1>, dim3(og), dim3(TPB), 0, c->stream, W);
        }
        int G = 2; // lanes per chain: the samples, rounded up to a power of two
        while (G < 64 && (u32)G < R.B.n_samples) G *= 2;
        // the counting pass of `index` leaves a margin in the item buffer: the insert pass packs its chunks in another order
        const u32 cap_eff = MODE == 1 ? W.item_cap / 8 * 7 : W.item_cap;
        if (c->use_chain_kernel && c->k >= 17 && c->k <= MG_MAX_PACKED_K) { // picks and evaluation in one kernel; what it lists, the pair below takes
            hipLaunchKernelGGL(fw_chain_kernel<MODE>, dim3(R.cus * 6), dim3(TPB), 0, c->stream, R.B, W, G, view(c, MG_BF_ALT), view(c), d_cov, d_overflow, d_cursor, row0,
                               d_evaluated);
            hipLaunchKernelGGL(fw_picks_kernel<true>, dim3(R.cus * 4), dim3(TPB), 0, c->stream, R.B, W, 64, cap_eff);
        } else {
            hipLaunchKernelGGL(fw_picks_kernel<false>, dim3(R.cus * 6), dim3(TPB), 0, c->stream, R.B, W, G, cap_eff);
            // (at G = 64 too: a chain that outgrew the whole set was LISTED by the launch above, and only this one hands its record on to
            //  tier 3 -- without it the record kept a coverage of zero and no flag: tests/test_gpu_block_edges.py C-share-40-385)
            hipLaunchKernelGGL(fw_picks_kernel<true>, dim3(R.cus * 4), dim3(TPB), 0, c->stream, R.B, W, 64, cap_eff);
        }
        hipLaunchKernelGGL(fw_eval_kernel<MODE>, dim3(R.cus * 8), dim3(TPB), 0, c->stream, R.B, W, view(c, MG_BF_ALT), view(c), d_cov, d_overflow, d_cursor, row0,
                           d_evaluated);
        hipLaunchKernelGGL(fw_slide_kernel<MODE>, dim3(R.cus * 8), dim3(TPB), 0, c->stream, R.B, W, view(c, MG_BF_ALT), view(c), d_cov, d_cursor, row0, d_evaluated);
        HIP_TRY(c, hipGetLastError());
    }
    return MG_OK;
}
// persistent grid of the workgroup kernel: as many workgroups as are resident together
template <int MODE> unsigned blocks_grid(mg_ctx *c)
{
    int &g = c->blocks_grid[MODE];
    if (!g) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cover_blocks_kernel<MODE>, TPB, 0) != hipSuccess || per_cu < 1) per_cu = 2;
        g = device_cus(c) * per_cu;
    }
    return (unsigned)g;
}
// tier 3: what tier 2 handed on, compacted, through the workgroup kernel; where it compacts, the caller has zeroed the list's count
// (c->d_gen_count[4]: blocks_clear, or a fill of its own; nothing but fb_compact_kernel writes it)
template <int MODE> int blocks_tier3(BlocksRun &R, bool compact, u32 *d_cov, u8 *d_overflow, unsigned long long *d_cursor, u32 row0, unsigned long long *d_evaluated)
{
    mg_ctx *c = R.c;
    unsigned long long *fb_count = c->d_gen_count + 4;
    if (compact) { // (the insert pass of `index` walks the counting pass's list)
        hipLaunchKernelGGL(fb_compact_kernel, dim3(R.cus * 8), dim3(TPB), 0, c->stream, (const u32 *)R.gen_list, (const unsigned long long *)c->d_gen_count,
                           (const u8 *)R.fb_flag, R.fb_list, fb_count);
    }
    hipLaunchKernelGGL(cover_blocks_kernel<MODE>, dim3(blocks_grid<MODE>(c)), dim3(TPB), 0, c->stream, R.B, (const u32 *)R.fb_list, (const unsigned long long *)fb_count,
                       view(c, MG_BF_ALT), view(c), d_cov, d_overflow, IndexEmit{nullptr, d_cursor, row0}, d_evaluated);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
} // namespace

// block cutting for a batch of kept records in file order (main.cpp:341, 547; var_block.hpp:77-80), on the device
MG_EXPORT int mg_cut_blocks_device(mg_ctx *c, const mg_panel_dev *p, void *d_blk_var_off_out, void *d_var_block_out, void *d_n_blocks_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_panel(c, p, false));
    if (!d_n_blocks_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (p->n_vars == 0) {
        HIP_TRY(c, hipMemsetAsync(d_n_blocks_out, 0, 8, c->stream));
        return MG_OK;
    }
    if (!d_blk_var_off_out) return fail(c, MG_ERR_ARG, "NULL argument");
    const u64 n = p->n_vars;
    void *d_cut, *d_ts;
    TRY(scratch(c, c->s_blk[9], n, &d_cut));
    TRY(scratch(c, c->s_blk[10], 4 * (u64)nblocks(n) + 4, &d_ts));
    hipLaunchKernelGGL(cut_flags_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, n, (const int *)p->pos, (const u32 *)p->ref_size, (const u32 *)p->min_size,
                       (const u32 *)p->contig_id, (int)c->k, (u8 *)d_cut, (u32 *)d_ts);
    return scan_flags(c, n, (const u8 *)d_cut, (u32 *)d_ts, (u32 *)d_blk_var_off_out, (u32 *)d_var_block_out, (unsigned long long *)d_n_blocks_out);
}

MG_EXPORT int mg_cut_blocks(mg_ctx *c, size_t n_vars, const int32_t *pos, const uint32_t *ref_size, const uint32_t *min_size, const uint32_t *contig_id,
                            uint32_t *blk_var_off_out, size_t *n_blocks_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (!n_blocks_out) return fail(c, MG_ERR_ARG, "NULL argument");
    *n_blocks_out = 0;
    if (n_vars == 0) return MG_OK;
    if (!pos || !ref_size || !min_size || !contig_id || !blk_var_off_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= 0xFFFFFFFFull) return fail(c, MG_ERR_LIMIT, "mg_cut_blocks takes fewer than 2^32 records per batch");
    void *d_pos, *d_rs, *d_ms, *d_cid, *d_off;
    TRY(upload(c, c->s_misc[0], pos, 4 * n_vars, &d_pos));
    TRY(upload(c, c->s_misc[1], ref_size, 4 * n_vars, &d_rs));
    TRY(upload(c, c->s_misc[2], min_size, 4 * n_vars, &d_ms));
    TRY(upload(c, c->s_misc[3], contig_id, 4 * n_vars, &d_cid));
    TRY(scratch(c, c->s_out, 4 * (n_vars + 1), &d_off));
    if (!c->d_gen_count) HIP_TRY(c, hipMalloc(&c->d_gen_count, 64));
    mg_panel_dev p{};
    p.n_vars = n_vars;
    p.pos = (const int32_t *)d_pos; p.ref_size = (const uint32_t *)d_rs; p.min_size = (const uint32_t *)d_ms; p.contig_id = (const uint32_t *)d_cid;
    TRY(mg_cut_blocks_device(c, &p, d_off, nullptr, c->d_gen_count + 1));
    unsigned long long nb = 0;
    HIP_TRY(c, hipMemcpyAsync(&nb, c->d_gen_count + 1, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(blk_var_off_out, d_off, 4 * (nb + 1), hipMemcpyDeviceToHost));
    *n_blocks_out = (size_t)nb;
    return MG_OK;
}

// VB::extract_kmers + set_coverages (main.cpp:556-557) for every block of a resident panel
MG_EXPORT int mg_cover_blocks_device(mg_ctx *c, const mg_panel_dev *p, const void *d_blk_var_off, const void *d_var_block, const void *d_n_blocks, int haploid,
                                     void *d_cov_out, void *d_overflow_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_panel(c, p, true));
    if (p->n_vars == 0) return MG_OK;
    if (!d_blk_var_off || !d_n_blocks || !d_cov_out || !d_overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    Timer &t = c->tm[TM_BLOCKS];
    TRY(timer_begin(c, t));
    BlocksRun R{};
    TRY(blocks_setup(c, p, (const u32 *)d_blk_var_off, (const u32 *)d_var_block, (const unsigned long long *)d_n_blocks, haploid, &R));
    const u64 n = p->n_vars;
    TRY(blocks_clear(R, (u8 *)d_overflow_out, c->d_gen_count, 8));
    // tier 1: lone and short records (classification fused in); everything else is listed
    u32 *need_slow = (u32 *)(c->d_hit_count + 3);
    if (++c->iso_call_no == 0) c->iso_call_no = 1;
    const int tiles = lone_tiles_for(c, 2 * n);
    const unsigned grid = lone_grid(2 * n, tiles);
    hipLaunchKernelGGL(panel_lone_kernel<false>, dim3(grid), dim3(TPB), 0, c->stream, R.P, n, R.B.blk_var_off, R.B.var_block, (const u8 *)c->d_ref,
                       (const u64 *)c->d_ref2, (const u32 *)c->d_refbad, (const u8 *)p->pool, (int)c->k, haploid, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, need_slow,
                       c->iso_call_no, R.gen_list, c->d_gen_count, (unsigned short *)R.B.rec_class, tiles);
    hipLaunchKernelGGL(panel_lone_kernel<true>, dim3(lone_slow_grid(c, grid)), dim3(TPB), 0, c->stream, R.P, n, R.B.blk_var_off, R.B.var_block, (const u8 *)c->d_ref,
                       (const u64 *)c->d_ref2, (const u32 *)c->d_refbad, (const u8 *)p->pool, (int)c->k, haploid, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, need_slow,
                       c->iso_call_no, R.gen_list, c->d_gen_count, (unsigned short *)R.B.rec_class, tiles);
    HIP_TRY(c, hipGetLastError());
    TRY(timer_mark(c, t, 1));
    TRY(blocks_tier2<0>(R, (u32 *)d_cov_out, (u8 *)d_overflow_out, nullptr, 0u, c->d_gen_count + 3));
    TRY(timer_mark(c, t, 2));
    TRY(blocks_tier3<0>(R, true, (u32 *)d_cov_out, (u8 *)d_overflow_out, nullptr, 0u, c->d_gen_count + 3));
    hipLaunchKernelGGL(fw_finish_kernel, dim3(R.cus * 8), dim3(TPB), 0, c->stream, R.B, (const u32 *)R.gen_list, (const unsigned long long *)c->d_gen_count,
                       (const u8 *)d_overflow_out, (u32 *)d_cov_out);
    HIP_TRY(c, hipGetLastError());
    return timer_mark(c, t, 3);
}

// The record loop for every plane of a cohort: tier 1 once over all planes (cohort_lone_kernel), tiers 2 and 3 plane by plane over the
// general list tier 1 wrote once.  (The chain walks are repeated per plane: fw_walk_kernel also clears the plane's coverages and
// reserves in the round's counter block what the kernels behind it consume, so a round's buffers serve one pass.)
namespace {
// slots = var_allele_off[n_vars], the distance between the planes of d_cov_out; 0: not known to the caller, read back from the device
int cover_cohort(mg_ctx *c, const mg_panel_dev *p, const void *d_blk_var_off, const void *d_var_block, const void *d_n_blocks, int haploid, void *d_cov_out,
                 void *d_overflow_out, u64 slots_known)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->coh_planes) return fail(c, MG_ERR_STATE, "mg_cover_blocks_cohort_device: not in cohort mode (mg_cohort_begin first)");
    TRY(check_panel(c, p, true));
    if (p->n_vars == 0) return MG_OK;
    if (!d_blk_var_off || !d_n_blocks || !d_cov_out || !d_overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    Timer &t = c->tm[TM_COHORT];
    TRY(timer_begin(c, t));
    c->tm[TM_BLOCKS].valid = false; // (mg_blocks_stats describes the single-sample call only)
    BlocksRun R{};
    TRY(blocks_setup(c, p, (const u32 *)d_blk_var_off, (const u32 *)d_var_block, (const unsigned long long *)d_n_blocks, haploid, &R));
    const u64 n = p->n_vars;
    u64 slots = slots_known; // the planes of d_cov_out are `slots` apart
    if (!slots) {
        u32 h_slots = 0;
        HIP_TRY(c, hipMemcpyAsync(&h_slots, p->var_allele_off + n, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        slots = h_slots;
    }
    TRY(blocks_clear(R, (u8 *)d_overflow_out, c->d_gen_count, 8)); // (with plane 0's flags and round counters)
    u32 *need_slow = (u32 *)(c->d_hit_count + 3);
    if (++c->iso_call_no == 0) c->iso_call_no = 1;
    const u32 sel = c->coh_sel;
    c->coh_sel = 0; // tier 1's views address plane 0: the kernel walks the cells from there
    const int tiles = lone_tiles_for(c, 2 * n);
    const unsigned grid = lone_grid(2 * n, tiles);
    hipLaunchKernelGGL(cohort_lone_kernel<false>, dim3(grid), dim3(TPB), 0, c->stream, R.P, n, R.B.blk_var_off, R.B.var_block, (const u8 *)c->d_ref, (const u64 *)c->d_ref2,
                       (const u32 *)c->d_refbad, (const u8 *)p->pool, (int)c->k, haploid, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, c->coh_planes, slots, need_slow,
                       c->iso_call_no, R.gen_list, c->d_gen_count, (unsigned short *)R.B.rec_class, tiles);
    hipLaunchKernelGGL(cohort_lone_kernel<true>, dim3(lone_slow_grid(c, grid)), dim3(TPB), 0, c->stream, R.P, n, R.B.blk_var_off, R.B.var_block, (const u8 *)c->d_ref, (const u64 *)c->d_ref2,
                       (const u32 *)c->d_refbad, (const u8 *)p->pool, (int)c->k, haploid, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, c->coh_planes, slots, need_slow,
                       c->iso_call_no, R.gen_list, c->d_gen_count, (unsigned short *)R.B.rec_class, tiles);
    int rc = hipGetLastError() == hipSuccess ? MG_OK : fail(c, MG_ERR_HIP, "cohort_lone_kernel launch failed");
    if (rc == MG_OK) rc = timer_mark(c, t, 1);
    for (u32 s = 0; s < c->coh_planes && rc == MG_OK; ++s) { // the other records, plane by plane, through the single-sample tiers
        c->coh_sel = s;
        u32 *cov = (u32 *)d_cov_out + (u64)s * slots;
        if (s) rc = blocks_clear(R, nullptr, c->d_gen_count + 3, 2); // the plane's own: flags, signature k-mers and tier 3's count, round counters
        if (rc == MG_OK) rc = blocks_tier2<0>(R, cov, (u8 *)d_overflow_out, nullptr, 0u, c->d_gen_count + 3);
        if (rc == MG_OK) rc = blocks_tier3<0>(R, true, cov, (u8 *)d_overflow_out, nullptr, 0u, c->d_gen_count + 3);
        if (rc != MG_OK) break;
        hipLaunchKernelGGL(fw_finish_kernel, dim3(R.cus * 8), dim3(TPB), 0, c->stream, R.B, (const u32 *)R.gen_list, (const unsigned long long *)c->d_gen_count,
                           (const u8 *)d_overflow_out, cov);
        if (hipGetLastError() != hipSuccess) rc = fail(c, MG_ERR_HIP, "fw_finish_kernel launch failed");
    }
    c->coh_sel = sel;
    TRY(rc);
    return timer_mark(c, t, 2);
}
} // namespace
MG_EXPORT int mg_cover_blocks_cohort_device(mg_ctx *c, const mg_panel_dev *p, const void *d_blk_var_off, const void *d_var_block, const void *d_n_blocks, int haploid,
                                            void *d_cov_out, void *d_overflow_out)
{
    return cover_cohort(c, p, d_blk_var_off, d_var_block, d_n_blocks, haploid, d_cov_out, d_overflow_out, 0);
}
// device milliseconds of the most recent mg_cover_blocks_cohort_device (waits for it): ms_out[0] tier 1 over all planes, [1] tiers 2-3 of all planes
MG_EXPORT int mg_cohort_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    if (!c->tm[TM_COHORT].valid) return fail(c, MG_ERR_STATE, "no mg_cover_blocks_cohort_device yet");
    return timer_read(c, c->tm[TM_COHORT], ms_out);
}

// ---- the rows of a merged batch: the sample columns as text (call_text_kernels.h), the site tags (site_tags_kernels.h), the sample columns
// ---- as BCF (bcf_kernels.h) ---------------------------------------------------------------------------------------------------------
namespace {
// A batch's cells are mg_cells (malva_hip.h) for every call of this section, the encoders' public one included: host pointers in a host
// form and device pointers in a device form, NULL where a call has no such array
inline bool has_gp(const mg_cells &x) { return x.fields & MG_CELLS_GP; }
inline bool has_pl(const mg_cells &x) { return x.fields & MG_CELLS_PL; }
// The argument checks that a host form and its device form share: of whoever reads a batch's cells (gq where reads_gq; an encoder: cov with
// var_allele_off or neither, and with gp var_allele_off with or without cov and the likelihoods), and of where an encoder's rows go
int check_cells(mg_ctx *c, const char *who, const mg_cells &x, bool encoder, bool reads_gq)
{
    const bool gp = has_gp(x), with_pl = has_pl(x);
    if (x.n_planes < 1 || x.n_planes > 64) return fail(c, MG_ERR_ARG, "%s: n_planes is 1..64", who);
    if (encoder && !gp && !with_pl && (x.cov != nullptr) != (x.var_allele_off != nullptr)) return fail(c, MG_ERR_ARG, "%s: cov and var_allele_off go together", who);
    if ((gp || with_pl) && (!x.var_allele_off || !x.var_gt_off)) return fail(c, MG_ERR_ARG, "%s: var_allele_off and var_gt_off are required", who);
    if (with_pl && (x.probs != nullptr) != (x.status != nullptr)) return fail(c, MG_ERR_ARG, "%s: probs and status go together", who);
    if (x.n_vars && (!x.gt1 || (!x.haploid && !x.gt2) || (reads_gq && !x.gq))) return fail(c, MG_ERR_ARG, "NULL argument");
    if (x.n_vars && gp && (!x.probs || !x.status)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (x.n_vars && with_pl && !x.pl) return fail(c, MG_ERR_ARG, "NULL argument");
    if (x.n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "%s: more than 2^32 - 1 records in one call", who);
    return MG_OK;
}
int check_rows_out(mg_ctx *c, const void *out, size_t cap, const void *row_off, const uint64_t *bytes_out)
{
    if (!row_off || !bytes_out || (!out && cap)) return fail(c, MG_ERR_ARG, "NULL argument");
    return MG_OK;
}

// row lengths -> row_off[n + 1] (u64) and, in meta[0], the total (~0 when meta[1] is set)
void fmt_scan(mg_ctx *c, const void *d_len, u64 n, u64 n_part, void *part, void *d_row_off, unsigned long long *meta)
{
    hipLaunchKernelGGL(tile_reduce_kernel, dim3((unsigned)n_part), dim3(SCAN_TPB), 0, c->stream, (const u32 *)d_len, n, (unsigned long long *)part);
    hipLaunchKernelGGL(part_scan_kernel, dim3(1), dim3(SCAN_TPB), 0, c->stream, (unsigned long long *)part, n_part, meta);
    hipLaunchKernelGGL(fmt_rescan_kernel, dim3((unsigned)n_part), dim3(SCAN_TPB), 0, c->stream, (const u32 *)d_len, n, (const unsigned long long *)part,
                       (unsigned long long *)d_row_off, meta);
}
inline dim3 fmt_len_grid(u64 n) { return dim3((unsigned)((n + FMT_TPB / 64 - 1) / (FMT_TPB / 64))); } // a wave per record
inline dim3 fmt_write_grid(u64 n) { return dim3((unsigned)((n + FMT_ROWS - 1) / FMT_ROWS)); }         // FMT_ROWS records per workgroup

// The device forms of the three encoders (enc: TM_FMT, TM_INFO, TM_BCF) differ in their two kernels alone: a length pass, the scan of the
// lengths into d_row_off[n_rows + 1], a write pass into d_out[cap], the four events of the stats call between them.  launch_len(len, meta)
// and launch_write(row_off) launch the encoder's kernel of that pass (launch_len may take scratch first, hence its return code).  More than
// cap bytes: MG_ERR_LIMIT with *bytes_out set, row_off whole, nothing written at or behind cap.
template <class LaunchLen, class LaunchWrite>
int encode_rows(mg_ctx *c, int enc, const char *who, size_t n_rows, void *d_out, size_t cap, void *d_row_off, uint64_t *bytes_out, LaunchLen launch_len,
                LaunchWrite launch_write)
{
    TRY(check_rows_out(c, d_out, cap, d_row_off, bytes_out));
    if (n_rows >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "%s: more than 2^32 - 1 records in one call", who); // (mg_format_site_info*: rows without cells)
    Timer &t = c->tm[enc];
    TRY(timer_begin(c, t));
    *bytes_out = 0;
    if (n_rows == 0) {
        HIP_TRY(c, hipMemsetAsync(d_row_off, 0, 8, c->stream));
        for (int i = 1; i < 4; ++i) TRY(timer_mark(c, t, i));
        return MG_OK;
    }
    void *d_len, *d_meta, *part;
    TRY(scratch(c, c->s_enc[enc][ES_LEN], 4 * n_rows, &d_len));
    TRY(scratch(c, c->s_enc[enc][ES_META], 16, &d_meta));
    const u64 n_part = (n_rows + SCAN_CHUNK - 1) / SCAN_CHUNK;
    TRY(scratch(c, c->s_scan, 8 * n_part, &part));
    unsigned long long *meta = (unsigned long long *)d_meta;
    HIP_TRY(c, hipMemsetAsync(d_meta, 0, 16, c->stream));
    TRY(launch_len((u32 *)d_len, meta));
    TRY(timer_mark(c, t, 1));
    fmt_scan(c, d_len, (u64)n_rows, n_part, part, d_row_off, meta);
    TRY(timer_mark(c, t, 2));
    launch_write((const unsigned long long *)d_row_off);
    HIP_TRY(c, hipGetLastError());
    TRY(timer_mark(c, t, 3));
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, d_meta, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (total == ~0ull) return fail(c, MG_ERR_LIMIT, "%s: a row of 4 GB or more", who);
    *bytes_out = total;
    if (total > cap) return fail(c, MG_ERR_LIMIT, "%s: the rows need %llu bytes, the buffer holds %llu", who, total, (unsigned long long)cap);
    return MG_OK;
}

// device milliseconds of an encoder's most recent call (waits for it): ms_out[0] length pass, [1] scan, [2] write pass
int rows_stats(mg_ctx *c, int enc, const char *who, float *ms_out)
{
    if (!c->tm[enc].valid) return fail(c, MG_ERR_STATE, "no %s yet", who);
    return timer_read(c, c->tm[enc], ms_out);
}

// The host forms' way in: a batch's cells go up, *d = h with device pointers.  gt1; gt2 unless haploid; gq where given and read (always, or
// under the mask alone); whatever else is given -- at n_vars == 0 only when_empty (the encoders and mg_pack_dosage, who take var_allele_off
// [0 .. n_vars] as it comes; mg_site_counts and mg_sample_counts do not read it then).  cov and allele_class are sized from
// var_allele_off[n_vars], probs and pl from var_gt_off[n_vars].  What is not uploaded is NULL on the device side.
int stage_cells(mg_ctx *c, const mg_cells &h, mg_cells *d, bool always_gq, bool when_empty)
{
    *d = h;
    const bool gp = has_gp(h), with_pl = has_pl(h);
    auto up = [&](int slot, const void *host, bool wanted, size_t bytes, const void **dev) -> int {
        void *p = nullptr;
        if (host && wanted) TRY(upload(c, c->stage[slot], host, bytes, &p));
        *dev = p;
        return MG_OK;
    };
    const bool rest = h.n_vars || when_empty;
    const size_t cells = (size_t)h.n_planes * h.n_vars, slots = h.var_allele_off && rest ? ((const uint32_t *)h.var_allele_off)[h.n_vars] : 0;
    TRY(up(ST_GT1, h.gt1, true, 4 * cells, &d->gt1));
    TRY(up(ST_GT2, h.gt2, !h.haploid, 4 * cells, &d->gt2));
    TRY(up(ST_GQ, h.gq, always_gq || h.use_mask, 4 * cells, &d->gq));
    TRY(up(ST_COV, h.cov, rest, 4 * (size_t)h.n_planes * slots, &d->cov));
    TRY(up(ST_VAR_ALLELE_OFF, h.var_allele_off, rest, 4 * (h.n_vars + 1), &d->var_allele_off));
    TRY(up(ST_PROBS, h.probs, gp, 8 * (size_t)h.n_planes * (gp ? ((const uint64_t *)h.var_gt_off)[h.n_vars] : 0), &d->probs));
    TRY(up(ST_VAR_GT_OFF, h.var_gt_off, gp || with_pl, 8 * (h.n_vars + 1), &d->var_gt_off));
    TRY(up(ST_PL, h.pl, with_pl, 4 * (size_t)h.n_planes * (with_pl ? ((const uint64_t *)h.var_gt_off)[h.n_vars] : 0), &d->pl));
    TRY(up(ST_STATUS, h.status, rest, cells, &d->status));
    return up(ST_ALLELE_CLASS, h.allele_class, rest, slots, &d->allele_class);
}
int stage_rows(mg_ctx *c, size_t n_rows, size_t cap, void **d_out, void **d_row_off)
{
    TRY(scratch(c, c->stage[ST_OUT], cap ? cap : 1, d_out));
    return scratch(c, c->stage[ST_ROW_OFF], 8 * (n_rows + 1), d_row_off);
}
// the host forms' way out, behind the device form that returned rc: row_off and the rows come down (rows that do not fit, MG_ERR_LIMIT with
// *bytes_out set: row_off and the first cap bytes are still the caller's)
int fetch_rows(mg_ctx *c, int rc, size_t n_rows, const void *d_out, const void *d_row_off, void *out, size_t cap, uint64_t *row_off_out, const uint64_t *bytes_out)
{
    if (rc != MG_OK && !(rc == MG_ERR_LIMIT && *bytes_out)) return rc;
    const size_t have = std::min<uint64_t>(*bytes_out, cap);
    HIP_TRY(c, hipMemcpyAsync(row_off_out, d_row_off, 8 * (n_rows + 1), hipMemcpyDeviceToHost, c->stream));
    if (have) HIP_TRY(c, hipMemcpyAsync(out, d_out, have, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

} // namespace
MG_EXPORT int mg_format_calls_device(mg_ctx *c, const mg_cells *cells, void *d_text_out, size_t text_cap, void *d_row_off_out, uint64_t *text_bytes_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !cells) return MG_ERR_ARG;
    const mg_cells &x = *cells;
    TRY(check_cells(c, "mg_format_calls", x, true, true));
    const FmtArgs a{(u64)x.n_vars, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, (const u32 *)x.cov, (const u32 *)x.var_allele_off,
                    x.use_mask, x.min_gq, (const double *)x.probs, (const u64 *)x.var_gt_off, (const u8 *)x.status, (const i32 *)x.pl};
    const bool gp = has_gp(x);
    const auto len_kernel = has_pl(x) ? (gp ? fmt_len_kernel<true, true> : fmt_len_kernel<false, true>) : gp ? fmt_len_kernel<true> : fmt_len_kernel<false>;
    const auto write_kernel = has_pl(x) ? (gp ? fmt_write_kernel<true, true> : fmt_write_kernel<false, true>) : gp ? fmt_write_kernel<true> : fmt_write_kernel<false>;
    return encode_rows(
        c, TM_FMT, "mg_format_calls", x.n_vars, d_text_out, text_cap, d_row_off_out, text_bytes_out,
        [&](u32 *len, unsigned long long *meta) -> int {
            hipLaunchKernelGGL(len_kernel, fmt_len_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, len, meta);
            return MG_OK;
        },
        [&](const unsigned long long *row_off) {
            hipLaunchKernelGGL(write_kernel, fmt_write_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, row_off, (char *)d_text_out, (u64)text_cap);
        });
}

MG_EXPORT int mg_format_calls(mg_ctx *c, const mg_cells *cells, char *text_out, size_t text_cap, uint64_t *row_off_out, uint64_t *text_bytes_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || !cells) return MG_ERR_ARG;
    const mg_cells &x = *cells;
    TRY(check_cells(c, "mg_format_calls", x, true, true));
    TRY(check_rows_out(c, text_out, text_cap, row_off_out, text_bytes_out));
    mg_cells d;
    void *d_text, *d_off;
    TRY(stage_cells(c, x, &d, true, true));
    TRY(stage_rows(c, x.n_vars, text_cap, &d_text, &d_off));
    const int rc = mg_format_calls_device(c, &d, d_text, text_cap, d_off, text_bytes_out);
    return fetch_rows(c, rc, x.n_vars, d_text, d_off, text_out, text_cap, row_off_out, text_bytes_out);
}

// device milliseconds of the most recent mg_format_calls* (rows_stats)
MG_EXPORT int mg_format_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    return rows_stats(c, TM_FMT, "mg_format_calls", ms_out);
}

namespace {
int site_counts_device(mg_ctx *c, const mg_cells &x, int accumulate, void *d_ac, void *d_ns)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_cells(c, "mg_site_counts", x, false, x.use_mask));
    if (x.n_vars && (!x.var_allele_off || !d_ns)) return fail(c, MG_ERR_ARG, "NULL argument"); // (d_ac may be: records without slots)
    TRY(timer_begin(c, c->tm[TM_SITE]));
    if (x.n_vars) {
        const SiteArgs a{(u64)x.n_vars, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, x.use_mask, x.min_gq,
                         (const u32 *)x.var_allele_off, accumulate};
        hipLaunchKernelGGL(site_count_kernel, fmt_len_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, (u32 *)d_ac, (u32 *)d_ns);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_SITE], 1);
}
} // namespace
MG_EXPORT int mg_site_counts_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                                    int32_t min_gq, const void *d_var_allele_off, int accumulate, void *d_ac, void *d_ns)
{
    return site_counts_device(c, mg_cells{n_vars, n_planes, haploid, d_gt1, d_gt2, d_gq, use_mask, min_gq, nullptr, d_var_allele_off}, accumulate, d_ac, d_ns);
}

MG_EXPORT int mg_site_counts(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                             int32_t min_gq, const uint32_t *var_allele_off, int accumulate, uint32_t *ac, uint32_t *ns)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const mg_cells x{n_vars, n_planes, haploid, gt1, gt2, gq, use_mask, min_gq, nullptr, var_allele_off};
    TRY(check_cells(c, "mg_site_counts", x, false, use_mask));
    if (n_vars && !var_allele_off) return fail(c, MG_ERR_ARG, "NULL argument");
    const size_t slots = n_vars ? var_allele_off[n_vars] : 0;
    if (n_vars && (!ns || (slots && !ac))) return fail(c, MG_ERR_ARG, "NULL argument");
    mg_cells d;
    void *d_ac, *d_ns;
    TRY(stage_cells(c, x, &d, false, false));
    TRY(scratch(c, c->stage[ST_AC], slots ? 4 * slots : 1, &d_ac));
    TRY(scratch(c, c->stage[ST_NS], n_vars ? 4 * n_vars : 1, &d_ns));
    if (accumulate && slots) HIP_TRY(c, hipMemcpyAsync(d_ac, ac, 4 * slots, hipMemcpyHostToDevice, c->stream));
    if (accumulate && n_vars) HIP_TRY(c, hipMemcpyAsync(d_ns, ns, 4 * n_vars, hipMemcpyHostToDevice, c->stream));
    TRY(site_counts_device(c, d, accumulate, d_ac, d_ns));
    if (slots) HIP_TRY(c, hipMemcpyAsync(ac, d_ac, 4 * slots, hipMemcpyDeviceToHost, c->stream));
    if (n_vars) HIP_TRY(c, hipMemcpyAsync(ns, d_ns, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_format_site_info_device(mg_ctx *c, size_t n_vars, const void *d_ac, const void *d_ns, const void *d_var_allele_off, void *d_text_out, size_t text_cap,
                                         void *d_row_off_out, uint64_t *text_bytes_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (n_vars && (!d_ns || !d_var_allele_off)) return fail(c, MG_ERR_ARG, "NULL argument");
    const InfoArgs a{(u64)n_vars, (const u32 *)d_ac, (const u32 *)d_ns, (const u32 *)d_var_allele_off};
    return encode_rows(
        c, TM_INFO, "mg_format_site_info", n_vars, d_text_out, text_cap, d_row_off_out, text_bytes_out,
        [&](u32 *len, unsigned long long *meta) -> int {
            hipLaunchKernelGGL(info_len_kernel, fmt_len_grid(n_vars), dim3(FMT_TPB), 0, c->stream, a, len, meta);
            return MG_OK;
        },
        [&](const unsigned long long *row_off) {
            hipLaunchKernelGGL(info_write_kernel, fmt_write_grid(n_vars), dim3(FMT_TPB), 0, c->stream, a, row_off, (char *)d_text_out, (u64)text_cap);
        });
}

MG_EXPORT int mg_format_site_info(mg_ctx *c, size_t n_vars, const uint32_t *ac, const uint32_t *ns, const uint32_t *var_allele_off, char *text_out, size_t text_cap,
                                  uint64_t *row_off_out, uint64_t *text_bytes_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_rows_out(c, text_out, text_cap, row_off_out, text_bytes_out));
    if (n_vars && (!ns || !var_allele_off || (var_allele_off[n_vars] && !ac))) return fail(c, MG_ERR_ARG, "NULL argument");
    void *d_ac, *d_ns, *d_vao, *d_text, *d_off;
    TRY(upload(c, c->stage[ST_AC], ac, n_vars ? 4 * (size_t)var_allele_off[n_vars] : 0, &d_ac));
    TRY(upload(c, c->stage[ST_NS], ns, 4 * n_vars, &d_ns));
    TRY(upload(c, c->stage[ST_VAR_ALLELE_OFF], var_allele_off, n_vars ? 4 * (n_vars + 1) : 0, &d_vao));
    TRY(stage_rows(c, n_vars, text_cap, &d_text, &d_off));
    const int rc = mg_format_site_info_device(c, n_vars, d_ac, d_ns, d_vao, d_text, text_cap, d_off, text_bytes_out);
    return fetch_rows(c, rc, n_vars, d_text, d_off, text_out, text_cap, row_off_out, text_bytes_out);
}

// device milliseconds (waits for them): ms_out[0] the most recent mg_site_counts*, [1] the most recent mg_format_site_info* (its three passes together); 0 where there was none
MG_EXPORT int mg_site_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    if (!c->tm[TM_SITE].valid && !c->tm[TM_INFO].valid) return fail(c, MG_ERR_STATE, "no mg_site_counts or mg_format_site_info yet");
    float info[3];
    TRY(timer_read(c, c->tm[TM_SITE], &ms_out[0]));
    TRY(timer_read(c, c->tm[TM_INFO], info));
    ms_out[1] = info[0] + info[1] + info[2];
    return MG_OK;
}

// ---- the pair table of a multi-sample call set (pair_kernels.h) ------------------------------------------------------------------------
namespace {
int pack_dosage_device(mg_ctx *c, const mg_cells &x, void *d_planes_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_cells(c, "mg_pack_dosage", x, false, x.use_mask));
    if (!x.var_allele_off) return fail(c, MG_ERR_ARG, "mg_pack_dosage: var_allele_off is required");
    if (x.n_vars && !d_planes_out) return fail(c, MG_ERR_ARG, "NULL argument");
    TRY(timer_begin(c, c->tm[TM_PACK]));
    if (x.n_vars) {
        const u64 n_words = ((u64)x.n_vars + 63) / 64;
        const PackArgs a{(u64)x.n_vars, n_words, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, x.use_mask, x.min_gq,
                         (const u32 *)x.var_allele_off};
        hipLaunchKernelGGL(pack_dosage_kernel, dim3((unsigned)((n_words + PACK_TPB / 64 - 1) / (PACK_TPB / 64)), x.n_planes), dim3(PACK_TPB), 0, c->stream, a,
                           (unsigned long long *)d_planes_out);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_PACK], 1);
}
} // namespace
MG_EXPORT int mg_pack_dosage_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                                    int32_t min_gq, const void *d_var_allele_off, void *d_planes_out)
{
    return pack_dosage_device(c, mg_cells{n_vars, n_planes, haploid, d_gt1, d_gt2, d_gq, use_mask, min_gq, nullptr, d_var_allele_off}, d_planes_out);
}

MG_EXPORT int mg_pack_dosage(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                             int32_t min_gq, const uint32_t *var_allele_off, uint64_t *planes_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const mg_cells x{n_vars, n_planes, haploid, gt1, gt2, gq, use_mask, min_gq, nullptr, var_allele_off};
    TRY(check_cells(c, "mg_pack_dosage", x, false, use_mask));
    if (!var_allele_off) return fail(c, MG_ERR_ARG, "mg_pack_dosage: var_allele_off is required");
    if (n_vars && !planes_out) return fail(c, MG_ERR_ARG, "NULL argument");
    const size_t out_bytes = 8 * (size_t)n_planes * 3 * ((n_vars + 63) / 64);
    mg_cells d;
    void *d_out;
    TRY(stage_cells(c, x, &d, false, true));
    TRY(scratch(c, c->stage[ST_PLANES], out_bytes ? out_bytes : 1, &d_out));
    TRY(pack_dosage_device(c, d, d_out));
    if (out_bytes) HIP_TRY(c, hipMemcpyAsync(planes_out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

namespace {
int check_pairs(mg_ctx *c, size_t n_words, const void *a, uint32_t n_a, const void *b, uint32_t n_b, const void *counts)
{
    if (n_a < 1 || n_a > 64 || n_b < 1 || n_b > 64) return fail(c, MG_ERR_ARG, "mg_pair_counts: n_a and n_b are 1..64");
    if (!b && n_b != n_a) return fail(c, MG_ERR_ARG, "mg_pair_counts: planes_b == NULL means B is A: n_b must equal n_a");
    if (!counts || (n_words && !a)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_words >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_pair_counts: more than 2^32 - 1 words in one call");
    return MG_OK;
}
// (the cut of the word axis into runs: pair_count_plan, count_plan.h)
} // namespace

MG_EXPORT int mg_pair_counts_device(mg_ctx *c, size_t n_words, const void *d_planes_a, uint32_t n_a, const void *d_planes_b, uint32_t n_b, int accumulate, void *d_counts)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_pairs(c, n_words, d_planes_a, n_a, d_planes_b, n_b, d_counts));
    TRY(timer_begin(c, c->tm[TM_PAIR]));
    if (!accumulate) HIP_TRY(c, hipMemsetAsync(d_counts, 0, 8 * (size_t)n_a * n_b * 9, c->stream));
    if (n_words) {
        const u32 tiles_i = (n_a + PAIR_TILE - 1) / PAIR_TILE, tiles_j = (n_b + PAIR_TILE - 1) / PAIR_TILE;
        const bool symmetric = !d_planes_b;
        u64 n_runs = 0;
        const u64 run = pair_count_plan((u64)n_words, symmetric ? tiles_i * (tiles_i + 1) / 2 : tiles_i * tiles_j, &n_runs);
        const PairArgs a{(u64)n_words, run, (const unsigned long long *)d_planes_a, (const unsigned long long *)(symmetric ? d_planes_a : d_planes_b), n_a, n_b, symmetric};
        hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)n_runs, tiles_j, tiles_i), dim3(PAIR_TPB), 0, c->stream, a, (unsigned long long *)d_counts);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_PAIR], 1);
}

MG_EXPORT int mg_pair_counts(mg_ctx *c, size_t n_words, const uint64_t *planes_a, uint32_t n_a, const uint64_t *planes_b, uint32_t n_b, int accumulate, uint64_t *counts)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_pairs(c, n_words, planes_a, n_a, planes_b, n_b, counts));
    const size_t count_bytes = 8 * (size_t)n_a * n_b * 9;
    void *da, *db = nullptr, *d_counts;
    TRY(upload(c, c->stage[ST_PA], planes_a, 8 * (size_t)n_a * 3 * n_words, &da));
    if (planes_b) TRY(upload(c, c->stage[ST_PB], planes_b, 8 * (size_t)n_b * 3 * n_words, &db));
    TRY(scratch(c, c->stage[ST_COUNTS], count_bytes, &d_counts));
    if (accumulate) HIP_TRY(c, hipMemcpyAsync(d_counts, counts, count_bytes, hipMemcpyHostToDevice, c->stream));
    TRY(mg_pair_counts_device(c, n_words, da, n_a, db, n_b, accumulate, d_counts));
    HIP_TRY(c, hipMemcpyAsync(counts, d_counts, count_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them): ms_out[0] the most recent mg_pack_dosage*, [1] the most recent mg_pair_counts*; 0 where there was none
MG_EXPORT int mg_pairs_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = ms_out[1] = 0.f; // (also where it fails)
    if (!c->tm[TM_PACK].valid && !c->tm[TM_PAIR].valid) return fail(c, MG_ERR_STATE, "no mg_pack_dosage or mg_pair_counts yet");
    TRY(timer_read(c, c->tm[TM_PACK], &ms_out[0]));
    return timer_read(c, c->tm[TM_PAIR], &ms_out[1]);
}

// ---- the per-sample table of a multi-sample call set (sample_kernels.h) -----------------------------------------------------------------
namespace {
int check_sample(mg_ctx *c, const mg_cells &x, const void *counts)
{
    TRY(check_cells(c, "mg_sample_counts", x, false, true)); // (gq: the histogram reads it, mask or none)
    if (!counts || (x.n_vars && !x.var_allele_off)) return fail(c, MG_ERR_ARG, "NULL argument");
    return MG_OK;
}
// (the cut of the records into runs: sample_count_plan, count_plan.h)

int sample_counts_device(mg_ctx *c, const mg_cells &x, int accumulate, void *d_counts)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_sample(c, x, d_counts));
    TRY(timer_begin(c, c->tm[TM_SAMPLE]));
    if (!accumulate) HIP_TRY(c, hipMemsetAsync(d_counts, 0, 8 * (size_t)x.n_planes * MG_SAMPLE_SLOTS, c->stream));
    if (x.n_vars) {
        u64 n_runs = 0;
        const u64 run = sample_count_plan((u64)x.n_vars, x.n_planes, &n_runs);
        const SampleArgs a{(u64)x.n_vars, run, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, x.use_mask, x.min_gq, (const u8 *)x.status,
                           (const u32 *)x.cov, (const u32 *)x.var_allele_off, (const u8 *)x.allele_class};
        hipLaunchKernelGGL(sample_count_kernel, dim3((unsigned)n_runs, x.n_planes), dim3(SAMPLE_TPB), 0, c->stream, a, (unsigned long long *)d_counts);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_SAMPLE], 1);
}
} // namespace
MG_EXPORT int mg_sample_counts_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                                      int32_t min_gq, const void *d_status, const void *d_cov, const void *d_var_allele_off, const void *d_allele_class, int accumulate,
                                      void *d_counts)
{
    const mg_cells x{n_vars, n_planes, haploid, d_gt1, d_gt2, d_gq, use_mask, min_gq, d_cov, d_var_allele_off, nullptr, nullptr, d_status, nullptr, d_allele_class};
    return sample_counts_device(c, x, accumulate, d_counts);
}

MG_EXPORT int mg_sample_counts(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                               int32_t min_gq, const uint8_t *status, const uint32_t *cov, const uint32_t *var_allele_off, const uint8_t *allele_class, int accumulate,
                               uint64_t *counts)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const mg_cells x{n_vars, n_planes, haploid, gt1, gt2, gq, use_mask, min_gq, cov, var_allele_off, nullptr, nullptr, status, nullptr, allele_class};
    TRY(check_sample(c, x, counts));
    const size_t count_bytes = 8 * (size_t)n_planes * MG_SAMPLE_SLOTS;
    mg_cells d;
    void *d_counts;
    TRY(stage_cells(c, x, &d, true, false));
    TRY(scratch(c, c->stage[ST_COUNTS], count_bytes, &d_counts));
    if (accumulate) HIP_TRY(c, hipMemcpyAsync(d_counts, counts, count_bytes, hipMemcpyHostToDevice, c->stream));
    TRY(sample_counts_device(c, d, accumulate, d_counts));
    HIP_TRY(c, hipMemcpyAsync(counts, d_counts, count_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them) of the most recent mg_sample_counts*
MG_EXPORT int mg_sample_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = 0.f; // (also where it fails)
    if (!c->tm[TM_SAMPLE].valid) return fail(c, MG_ERR_STATE, "no mg_sample_counts yet");
    return timer_read(c, c->tm[TM_SAMPLE], ms_out);
}

// ---- the per-record table of a multi-sample call set (site_geno_kernels.h) ---------------------------------------------------------------
namespace {
int site_geno_counts_device(mg_ctx *c, const mg_cells &x, int accumulate, void *d_n, void *d_het, void *d_hom)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_cells(c, "mg_site_geno_counts", x, false, x.use_mask));
    if (x.n_vars && (!x.var_allele_off || !d_n)) return fail(c, MG_ERR_ARG, "NULL argument"); // (d_het and d_hom may be: records without slots)
    TRY(timer_begin(c, c->tm[TM_GENO]));
    if (x.n_vars) {
        const SiteArgs a{(u64)x.n_vars, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, x.use_mask, x.min_gq,
                         (const u32 *)x.var_allele_off, accumulate};
        hipLaunchKernelGGL(site_geno_kernel, fmt_len_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, (u32 *)d_n, (u32 *)d_het, (u32 *)d_hom);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_GENO], 1);
}
} // namespace
MG_EXPORT int mg_site_geno_counts_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                                         int32_t min_gq, const void *d_var_allele_off, int accumulate, void *d_n_out, void *d_het_out, void *d_hom_out)
{
    return site_geno_counts_device(c, mg_cells{n_vars, n_planes, haploid, d_gt1, d_gt2, d_gq, use_mask, min_gq, nullptr, d_var_allele_off}, accumulate, d_n_out, d_het_out,
                                   d_hom_out);
}

MG_EXPORT int mg_site_geno_counts(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                                  int32_t min_gq, const uint32_t *var_allele_off, int accumulate, uint32_t *n_out, uint32_t *het_out, uint32_t *hom_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const mg_cells x{n_vars, n_planes, haploid, gt1, gt2, gq, use_mask, min_gq, nullptr, var_allele_off};
    TRY(check_cells(c, "mg_site_geno_counts", x, false, use_mask));
    if (n_vars && !var_allele_off) return fail(c, MG_ERR_ARG, "NULL argument");
    const size_t slots = n_vars ? var_allele_off[n_vars] : 0;
    if (n_vars && (!n_out || (slots && (!het_out || !hom_out)))) return fail(c, MG_ERR_ARG, "NULL argument");
    mg_cells d;
    void *d_n, *d_het, *d_hom;
    TRY(stage_cells(c, x, &d, false, false));
    TRY(scratch(c, c->stage[ST_SG_N], n_vars ? 4 * n_vars : 1, &d_n));
    TRY(scratch(c, c->stage[ST_SG_HET], slots ? 4 * slots : 1, &d_het));
    TRY(scratch(c, c->stage[ST_SG_HOM], slots ? 4 * slots : 1, &d_hom));
    if (accumulate && n_vars) HIP_TRY(c, hipMemcpyAsync(d_n, n_out, 4 * n_vars, hipMemcpyHostToDevice, c->stream));
    if (accumulate && slots) HIP_TRY(c, hipMemcpyAsync(d_het, het_out, 4 * slots, hipMemcpyHostToDevice, c->stream));
    if (accumulate && slots) HIP_TRY(c, hipMemcpyAsync(d_hom, hom_out, 4 * slots, hipMemcpyHostToDevice, c->stream));
    TRY(site_geno_counts_device(c, d, accumulate, d_n, d_het, d_hom));
    if (n_vars) HIP_TRY(c, hipMemcpyAsync(n_out, d_n, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    if (slots) HIP_TRY(c, hipMemcpyAsync(het_out, d_het, 4 * slots, hipMemcpyDeviceToHost, c->stream));
    if (slots) HIP_TRY(c, hipMemcpyAsync(hom_out, d_hom, 4 * slots, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_hwe_exact_device(mg_ctx *c, size_t n_items, const void *d_n, const void *d_het, const void *d_hom, void *d_hwe_out, void *d_exc_het_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (n_items && (!d_n || !d_het || !d_hom || !d_hwe_out || !d_exc_het_out)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_items >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_hwe_exact: more than 2^32 - 1 items in one call");
    TRY(timer_begin(c, c->tm[TM_HWE]));
    if (n_items) {
        hipLaunchKernelGGL(hwe_exact_kernel, dim3((unsigned)((n_items + HWE_TPB - 1) / HWE_TPB)), dim3(HWE_TPB), 0, c->stream, (u64)n_items, (const u32 *)d_n,
                           (const u32 *)d_het, (const u32 *)d_hom, (double *)d_hwe_out, (double *)d_exc_het_out);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_HWE], 1);
}

MG_EXPORT int mg_hwe_exact(mg_ctx *c, size_t n_items, const uint32_t *n, const uint32_t *het, const uint32_t *hom, double *hwe_out, double *exc_het_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_items && (!n || !het || !hom || !hwe_out || !exc_het_out)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_items >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_hwe_exact: more than 2^32 - 1 items in one call");
    void *d_n, *d_het, *d_hom, *d_hwe, *d_exc;
    TRY(upload(c, c->stage[ST_SG_N], n, 4 * n_items, &d_n));
    TRY(upload(c, c->stage[ST_SG_HET], het, 4 * n_items, &d_het));
    TRY(upload(c, c->stage[ST_SG_HOM], hom, 4 * n_items, &d_hom));
    TRY(scratch(c, c->stage[ST_HWE], n_items ? 8 * n_items : 1, &d_hwe));
    TRY(scratch(c, c->stage[ST_EXC_HET], n_items ? 8 * n_items : 1, &d_exc));
    TRY(mg_hwe_exact_device(c, n_items, d_n, d_het, d_hom, d_hwe, d_exc));
    if (n_items) HIP_TRY(c, hipMemcpyAsync(hwe_out, d_hwe, 8 * n_items, hipMemcpyDeviceToHost, c->stream));
    if (n_items) HIP_TRY(c, hipMemcpyAsync(exc_het_out, d_exc, 8 * n_items, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them): ms_out[0] the most recent mg_site_geno_counts*, [1] the most recent mg_hwe_exact*; 0 where there was none
MG_EXPORT int mg_hwe_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = ms_out[1] = 0.f; // (also where it fails)
    if (!c->tm[TM_GENO].valid && !c->tm[TM_HWE].valid) return fail(c, MG_ERR_STATE, "no mg_site_geno_counts or mg_hwe_exact yet");
    TRY(timer_read(c, c->tm[TM_GENO], &ms_out[0]));
    return timer_read(c, c->tm[TM_HWE], &ms_out[1]);
}

// ---- the LD table of a multi-sample call set (ld_kernels.h) ---------------------------------------------------------------------------
namespace {
int pack_site_dosage_device(mg_ctx *c, const mg_cells &x, void *d_sites_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_cells(c, "mg_pack_site_dosage", x, false, x.use_mask));
    if (!x.var_allele_off) return fail(c, MG_ERR_ARG, "mg_pack_site_dosage: var_allele_off is required");
    if (x.n_vars && !d_sites_out) return fail(c, MG_ERR_ARG, "NULL argument");
    TRY(timer_begin(c, c->tm[TM_LD_PACK]));
    if (x.n_vars) {
        const PackArgs a{(u64)x.n_vars, 0, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, x.use_mask, x.min_gq,
                         (const u32 *)x.var_allele_off};
        hipLaunchKernelGGL(pack_site_kernel, dim3((unsigned)(((u64)x.n_vars + LD_PACK_RECS - 1) / LD_PACK_RECS)), dim3(LD_PACK_TPB), 0, c->stream, a,
                           (unsigned long long *)d_sites_out);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_LD_PACK], 1);
}
int check_ld(mg_ctx *c, size_t n_vars, size_t n_first, uint32_t n_groups, const void *sites, const void *chrom, const void *pos, uint32_t window, uint32_t min_n,
             double min_r2, const void *pairs_out, size_t pairs_cap, const void *row_off_out, const uint64_t *n_pairs_out)
{
    if (n_groups < 1 || n_groups > MG_LD_MAX_GROUPS) return fail(c, MG_ERR_ARG, "mg_ld_window: n_groups is 1..%d", MG_LD_MAX_GROUPS);
    if (window < 1 || window > MG_LD_MAX_WINDOW) return fail(c, MG_ERR_ARG, "mg_ld_window: window is 1..%d", MG_LD_MAX_WINDOW);
    if (!(min_r2 >= 0.0 && min_r2 <= 1.0)) return fail(c, MG_ERR_ARG, "mg_ld_window: min_r2 is in [0, 1]"); // (a NaN fails both)
    if (min_n < 1) return fail(c, MG_ERR_ARG, "mg_ld_window: min_n is at least 1");
    if (n_first > n_vars) return fail(c, MG_ERR_ARG, "mg_ld_window: n_first beyond n_vars");
    if (!row_off_out || !n_pairs_out || (!pairs_out && pairs_cap) || (n_vars && (!sites || !chrom || !pos))) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_ld_window: more than 2^32 - 1 records in one call");
    return MG_OK;
}
} // namespace
MG_EXPORT int mg_pack_site_dosage_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                                         int32_t min_gq, const void *d_var_allele_off, void *d_sites_out)
{
    return pack_site_dosage_device(c, mg_cells{n_vars, n_planes, haploid, d_gt1, d_gt2, d_gq, use_mask, min_gq, nullptr, d_var_allele_off}, d_sites_out);
}

MG_EXPORT int mg_pack_site_dosage(mg_ctx *c, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                                  int32_t min_gq, const uint32_t *var_allele_off, uint64_t *sites_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const mg_cells x{n_vars, n_planes, haploid, gt1, gt2, gq, use_mask, min_gq, nullptr, var_allele_off};
    TRY(check_cells(c, "mg_pack_site_dosage", x, false, use_mask));
    if (!var_allele_off) return fail(c, MG_ERR_ARG, "mg_pack_site_dosage: var_allele_off is required");
    if (n_vars && !sites_out) return fail(c, MG_ERR_ARG, "NULL argument");
    const size_t out_bytes = 8 * 3 * n_vars;
    mg_cells d;
    void *d_out;
    TRY(stage_cells(c, x, &d, false, true));
    TRY(scratch(c, c->stage[ST_LD_WORDS], out_bytes ? out_bytes : 1, &d_out));
    TRY(pack_site_dosage_device(c, d, d_out));
    if (out_bytes) HIP_TRY(c, hipMemcpyAsync(sites_out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// a length pass, the scan of the lengths into d_row_off[n_first + 1], a write pass that makes the same pairs again (ld_kernels.h); the
// total comes back between the scan and the return, as an encoder's does
MG_EXPORT int mg_ld_window_device(mg_ctx *c, size_t n_vars, size_t n_first, uint32_t n_groups, const void *d_sites, const void *d_chrom, const void *d_pos,
                                  uint32_t window, uint64_t max_bp, uint32_t min_n, double min_r2, void *d_pairs_out, size_t pairs_cap, void *d_row_off_out,
                                  uint64_t *n_pairs_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_ld(c, n_vars, n_first, n_groups, d_sites, d_chrom, d_pos, window, min_n, min_r2, d_pairs_out, pairs_cap, d_row_off_out, n_pairs_out));
    Timer &t = c->tm[TM_LD];
    TRY(timer_begin(c, t));
    *n_pairs_out = 0;
    if (n_first == 0) {
        HIP_TRY(c, hipMemsetAsync(d_row_off_out, 0, 8, c->stream));
        for (int i = 1; i < 4; ++i) TRY(timer_mark(c, t, i));
        return MG_OK;
    }
    void *d_len, *d_meta, *part;
    TRY(scratch(c, c->s_ld[0], 4 * n_first, &d_len));
    TRY(scratch(c, c->s_ld[1], 16, &d_meta));
    const u64 n_part = ((u64)n_first + SCAN_CHUNK - 1) / SCAN_CHUNK;
    TRY(scratch(c, c->s_scan, 8 * n_part, &part));
    unsigned long long *meta = (unsigned long long *)d_meta;
    HIP_TRY(c, hipMemsetAsync(d_meta, 0, 16, c->stream));
    const LdArgs a{(u64)n_vars, (u64)n_first, n_groups, window, (const unsigned long long *)d_sites, (const u32 *)d_chrom, (const u32 *)d_pos, max_bp, min_n, min_r2};
    const dim3 grid((unsigned)(((u64)n_first + LD_TILE - 1) / LD_TILE));
    hipLaunchKernelGGL(ld_window_kernel<false>, grid, dim3(LD_TPB), 0, c->stream, a, (u32 *)d_len, (const unsigned long long *)nullptr, (LdPair *)nullptr, (u64)0);
    HIP_TRY(c, hipGetLastError());
    TRY(timer_mark(c, t, 1));
    fmt_scan(c, d_len, (u64)n_first, n_part, part, d_row_off_out, meta);
    HIP_TRY(c, hipGetLastError());
    TRY(timer_mark(c, t, 2));
    hipLaunchKernelGGL(ld_window_kernel<true>, grid, dim3(LD_TPB), 0, c->stream, a, (u32 *)nullptr, (const unsigned long long *)d_row_off_out, (LdPair *)d_pairs_out,
                       (u64)pairs_cap);
    HIP_TRY(c, hipGetLastError());
    TRY(timer_mark(c, t, 3));
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, d_meta, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_pairs_out = total;
    if (total > pairs_cap) return fail(c, MG_ERR_LIMIT, "mg_ld_window: %llu pairs, the buffer holds %llu", total, (unsigned long long)pairs_cap);
    return MG_OK;
}

MG_EXPORT int mg_ld_window(mg_ctx *c, size_t n_vars, size_t n_first, uint32_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, uint32_t window,
                           uint64_t max_bp, uint32_t min_n, double min_r2, mg_ld_pair *pairs_out, size_t pairs_cap, uint64_t *row_off_out, uint64_t *n_pairs_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_ld(c, n_vars, n_first, n_groups, sites, chrom, pos, window, min_n, min_r2, pairs_out, pairs_cap, row_off_out, n_pairs_out));
    void *d_sites, *d_chrom, *d_pos, *d_pairs, *d_off;
    TRY(upload(c, c->stage[ST_LD_SITES], sites, 8 * (size_t)n_groups * 3 * n_vars, &d_sites));
    TRY(upload(c, c->stage[ST_LD_CHROM], chrom, 4 * n_vars, &d_chrom));
    TRY(upload(c, c->stage[ST_LD_POS], pos, 4 * n_vars, &d_pos));
    TRY(scratch(c, c->stage[ST_LD_PAIRS], pairs_cap ? sizeof(mg_ld_pair) * pairs_cap : 1, &d_pairs));
    TRY(scratch(c, c->stage[ST_LD_ROW_OFF], 8 * (n_first + 1), &d_off));
    const int rc = mg_ld_window_device(c, n_vars, n_first, n_groups, d_sites, d_chrom, d_pos, window, max_bp, min_n, min_r2, d_pairs, pairs_cap, d_off, n_pairs_out);
    if (rc != MG_OK && !(rc == MG_ERR_LIMIT && *n_pairs_out > pairs_cap)) return rc;
    const size_t have = std::min<uint64_t>(*n_pairs_out, pairs_cap);
    HIP_TRY(c, hipMemcpyAsync(row_off_out, d_off, 8 * (n_first + 1), hipMemcpyDeviceToHost, c->stream));
    if (have) HIP_TRY(c, hipMemcpyAsync(pairs_out, d_pairs, sizeof(mg_ld_pair) * have, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

// device milliseconds (waits for them): ms_out[0] the most recent mg_pack_site_dosage*, [1] the most recent mg_ld_window* (its three passes together); 0 where there was none
MG_EXPORT int mg_ld_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = ms_out[1] = 0.f; // (also where it fails)
    if (!c->tm[TM_LD_PACK].valid && !c->tm[TM_LD].valid) return fail(c, MG_ERR_STATE, "no mg_pack_site_dosage or mg_ld_window yet");
    float passes[3];
    TRY(timer_read(c, c->tm[TM_LD_PACK], &ms_out[0]));
    TRY(timer_read(c, c->tm[TM_LD], passes));
    ms_out[1] = passes[0] + passes[1] + passes[2];
    return MG_OK;
}

// ---- IBS0-free segments per pair of samples (ibd_kernels.h) ---------------------------------------------------------------------------
namespace {
int check_sites_to_planes(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *sites, const void *planes_out)
{
    if (n_groups < 1 || n_groups > MG_LD_MAX_GROUPS) return fail(c, MG_ERR_ARG, "mg_sites_to_planes: n_groups is 1..%d", MG_LD_MAX_GROUPS);
    if (n_vars && (!sites || !planes_out)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_sites_to_planes: more than 2^32 - 1 records in one call");
    return MG_OK;
}
int check_ibd_step(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *sites, const void *chrom, const void *pos, const void *segs_out, size_t segs_cap,
                   const uint64_t *n_segs_out)
{
    if (!c->ibd_state) return fail(c, MG_ERR_STATE, "mg_ibd_step: no mg_ibd_begin yet");
    if (n_groups != (c->ibd_samples + 63) / 64) return fail(c, MG_ERR_ARG, "mg_ibd_step: n_groups is ceil(n_samples / 64) = %u", (c->ibd_samples + 63) / 64);
    if (!n_segs_out || (!segs_out && segs_cap) || (n_vars && (!sites || !chrom || !pos))) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_ibd_step: more than 2^32 - 1 records in one call");
    return MG_OK;
}
void ibd_drop(mg_ctx *c)
{
    if (c->ibd_state) hipFree(c->ibd_state);
    c->ibd_state = nullptr;
    c->ibd_pairs = 0;
    c->ibd_samples = 0;
}
} // namespace

MG_EXPORT int mg_sites_to_planes_device(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *d_sites, void *d_planes_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_sites_to_planes(c, n_vars, n_groups, d_sites, d_planes_out));
    TRY(timer_begin(c, c->tm[TM_IBD_TR]));
    if (n_vars) {
        const u64 n_words = ((u64)n_vars + 63) / 64;
        hipLaunchKernelGGL(sites_to_planes_kernel, dim3((unsigned)((n_words + IBD_TR_WORDS - 1) / IBD_TR_WORDS), 3, n_groups), dim3(IBD_TR_TPB), 0, c->stream,
                           (const unsigned long long *)d_sites, (u64)n_vars, n_words, (unsigned long long *)d_planes_out);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_IBD_TR], 1);
}

MG_EXPORT int mg_sites_to_planes(mg_ctx *c, size_t n_vars, uint32_t n_groups, const uint64_t *sites, uint64_t *planes_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_sites_to_planes(c, n_vars, n_groups, sites, planes_out));
    const size_t in_bytes = 8 * (size_t)n_groups * 3 * n_vars, out_bytes = 8 * 64 * (size_t)n_groups * 3 * ((n_vars + 63) / 64);
    void *d_sites, *d_planes;
    TRY(upload(c, c->stage[ST_IBD_SITES], sites, in_bytes, &d_sites));
    TRY(scratch(c, c->stage[ST_IBD_PLANES], out_bytes ? out_bytes : 1, &d_planes));
    TRY(mg_sites_to_planes_device(c, n_vars, n_groups, d_sites, d_planes));
    if (out_bytes) HIP_TRY(c, hipMemcpyAsync(planes_out, d_planes, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_ibd_begin(mg_ctx *c, uint32_t n_samples, uint32_t min_records, uint64_t min_bp)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_samples < 2 || n_samples > MG_IBD_MAX_SAMPLES) return fail(c, MG_ERR_ARG, "mg_ibd_begin: n_samples is 2..%d", MG_IBD_MAX_SAMPLES);
    if (min_records < 1) return fail(c, MG_ERR_ARG, "mg_ibd_begin: min_records is at least 1");
    if (min_bp > (uint64_t)INT64_MAX) return fail(c, MG_ERR_ARG, "mg_ibd_begin: min_bp is at most 2^63 - 1");
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a step of the state that goes may still run)
    ibd_drop(c);
    const u64 n_pairs = (u64)n_samples * (n_samples - 1) / 2;
    const size_t bytes = 4 * IBD_FIELDS * n_pairs + 4; // every pair closed (n == 0); the last chrom id, which no closed pair asks for
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MG_ERR_NOMEM, "mg_ibd_begin: the state of %llu pairs (%zu bytes) does not fit", (unsigned long long)n_pairs, bytes);
    }
    c->ibd_state = (u32 *)p;
    c->ibd_pairs = n_pairs;
    c->ibd_samples = n_samples;
    c->ibd_min_records = min_records;
    c->ibd_min_bp = (long long)min_bp;
    HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->stream));
    return MG_OK;
}

MG_EXPORT int mg_ibd_end(mg_ctx *c)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ibd_drop(c);
    return MG_OK;
}

// the transpose and the start words; a length pass, the scan of the pairs' counts, the total read back; then, when the buffer holds it,
// the write pass, which also stores the state, and the last record's chrom id (ibd_kernels.h)
MG_EXPORT int mg_ibd_step_device(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *d_sites, const void *d_chrom, const void *d_pos, int flush, void *d_segs_out,
                                 size_t segs_cap, uint64_t *n_segs_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_ibd_step(c, n_vars, n_groups, d_sites, d_chrom, d_pos, d_segs_out, segs_cap, n_segs_out));
    Timer &t = c->tm[TM_IBD];
    TRY(timer_begin(c, t));
    *n_segs_out = 0;
    if (!n_vars && !flush) return timer_mark(c, t, 1);
    const u64 n_words = ((u64)n_vars + 63) / 64, n_pairs = c->ibd_pairs;
    u32 *d_last = c->ibd_state + IBD_FIELDS * n_pairs;
    void *d_planes = nullptr, *d_starts = nullptr, *d_len, *d_off, *d_meta, *part;
    if (n_vars) {
        TRY(scratch(c, c->s_ibd[0], 8 * 64 * (size_t)n_groups * 3 * n_words, &d_planes));
        TRY(scratch(c, c->s_ibd[1], 8 * n_words, &d_starts));
        TRY(mg_sites_to_planes_device(c, n_vars, n_groups, d_sites, d_planes));
        hipLaunchKernelGGL(ibd_starts_kernel, dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, c->stream, (const u32 *)d_chrom, (u64)n_vars, n_words,
                           (const u32 *)d_last, (unsigned long long *)d_starts);
        HIP_TRY(c, hipGetLastError());
    }
    TRY(scratch(c, c->s_ibd[2], 4 * n_pairs, &d_len));
    TRY(scratch(c, c->s_ibd[3], 8 * (n_pairs + 1), &d_off));
    TRY(scratch(c, c->s_ibd[4], 16, &d_meta));
    const u64 n_part = (n_pairs + SCAN_CHUNK - 1) / SCAN_CHUNK;
    TRY(scratch(c, c->s_scan, 8 * n_part, &part));
    HIP_TRY(c, hipMemsetAsync(d_meta, 0, 16, c->stream));
    const IbdArgs a{(u64)n_vars, n_words, n_pairs, c->ibd_samples, (const unsigned long long *)d_planes, (const unsigned long long *)d_starts, (const u32 *)d_chrom,
                    (const u32 *)d_pos, c->ibd_state, c->ibd_min_records, c->ibd_min_bp, flush != 0};
    const unsigned tiles = (c->ibd_samples + PAIR_TILE - 1) / PAIR_TILE;
    hipLaunchKernelGGL(ibd_walk_kernel<false>, dim3(tiles, tiles), dim3(PAIR_TPB), 0, c->stream, a, (u32 *)d_len, (const unsigned long long *)nullptr, (IbdSeg *)nullptr);
    HIP_TRY(c, hipGetLastError());
    fmt_scan(c, d_len, n_pairs, n_part, part, d_off, (unsigned long long *)d_meta);
    HIP_TRY(c, hipGetLastError());
    unsigned long long total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, d_meta, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_segs_out = total;
    if (total > segs_cap) {
        TRY(timer_mark(c, t, 1));
        return fail(c, MG_ERR_LIMIT, "mg_ibd_step: %llu segments, the buffer holds %llu", total, (unsigned long long)segs_cap);
    }
    hipLaunchKernelGGL(ibd_walk_kernel<true>, dim3(tiles, tiles), dim3(PAIR_TPB), 0, c->stream, a, (u32 *)nullptr, (const unsigned long long *)d_off, (IbdSeg *)d_segs_out);
    HIP_TRY(c, hipGetLastError());
    if (n_vars) HIP_TRY(c, hipMemcpyAsync(d_last, (const u32 *)d_chrom + (n_vars - 1), 4, hipMemcpyDeviceToDevice, c->stream));
    return timer_mark(c, t, 1);
}

MG_EXPORT int mg_ibd_step(mg_ctx *c, size_t n_vars, uint32_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, int flush, mg_ibd_seg *segs_out,
                          size_t segs_cap, uint64_t *n_segs_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_ibd_step(c, n_vars, n_groups, sites, chrom, pos, segs_out, segs_cap, n_segs_out));
    void *d_sites, *d_chrom, *d_pos, *d_segs;
    TRY(upload(c, c->stage[ST_IBD_SITES], sites, 8 * (size_t)n_groups * 3 * n_vars, &d_sites));
    TRY(upload(c, c->stage[ST_IBD_CHROM], chrom, 4 * n_vars, &d_chrom));
    TRY(upload(c, c->stage[ST_IBD_POS], pos, 4 * n_vars, &d_pos));
    TRY(scratch(c, c->stage[ST_IBD_SEGS], segs_cap ? sizeof(mg_ibd_seg) * segs_cap : 1, &d_segs));
    TRY(mg_ibd_step_device(c, n_vars, n_groups, d_sites, d_chrom, d_pos, flush, d_segs, segs_cap, n_segs_out));
    if (*n_segs_out) HIP_TRY(c, hipMemcpyAsync(segs_out, d_segs, sizeof(mg_ibd_seg) * *n_segs_out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them): ms_out[0] the most recent transpose, [1] the most recent step; 0 where there was none
MG_EXPORT int mg_ibd_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = ms_out[1] = 0.f; // (also where it fails)
    if (!c->tm[TM_IBD_TR].valid && !c->tm[TM_IBD].valid) return fail(c, MG_ERR_STATE, "no mg_sites_to_planes or mg_ibd_step yet");
    TRY(timer_read(c, c->tm[TM_IBD_TR], &ms_out[0]));
    return timer_read(c, c->tm[TM_IBD], &ms_out[1]);
}

// ---- the genetic relationship matrix (grm_kernels.h) ------------------------------------------------------------------------------------
namespace {
int check_grm_weights(mg_ctx *c, size_t n_vars, uint32_t n_groups, uint32_t n_samples, const void *sites, uint32_t maf_ppm, uint32_t min_n, const void *q_out)
{
    if (n_samples < 1 || n_samples > MG_GRM_MAX_SAMPLES) return fail(c, MG_ERR_ARG, "mg_grm: n_samples is 1..%d", MG_GRM_MAX_SAMPLES);
    if (n_groups != (n_samples + 63) / 64) return fail(c, MG_ERR_ARG, "mg_grm: n_groups is ceil(n_samples / 64) = %u", (n_samples + 63) / 64);
    if (maf_ppm > 500000) return fail(c, MG_ERR_ARG, "mg_grm: maf_ppm is 0..500000");
    if (min_n < 1) return fail(c, MG_ERR_ARG, "mg_grm: min_n is at least 1");
    if (n_vars && (!sites || !q_out)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_grm: more than 2^32 - 1 records in one call");
    return MG_OK;
}
int check_grm_step(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *sites)
{
    if (!c->grm_state) return fail(c, MG_ERR_STATE, "mg_grm_step: no mg_grm_begin yet");
    if (n_groups != (c->grm_samples + 63) / 64) return fail(c, MG_ERR_ARG, "mg_grm_step: n_groups is ceil(n_samples / 64) = %u", (c->grm_samples + 63) / 64);
    if (n_vars && !sites) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_grm_step: more than 2^32 - 1 records in one call");
    return MG_OK;
}
void grm_drop(mg_ctx *c)
{
    if (c->grm_state) hipFree(c->grm_state);
    c->grm_state = nullptr;
    c->grm_pairs = c->grm_seen = 0;
    c->grm_samples = 0;
}
void grm_launch_weights(mg_ctx *c, u64 n_vars, u64 v0, u64 count, u32 n_groups, u32 n_samples, const void *d_sites, int haploid, u32 maf_ppm, u32 min_n, void *d_q,
                        unsigned long long *d_entered)
{
    const GrmWeightArgs a{n_vars, v0, count, n_groups, n_samples, (const unsigned long long *)d_sites, haploid != 0, maf_ppm, min_n};
    hipLaunchKernelGGL(grm_weights_kernel, dim3((unsigned)((count + GRM_TPB - 1) / GRM_TPB)), dim3(GRM_TPB), 0, c->stream, a, (short4 *)d_q, d_entered);
}
} // namespace

MG_EXPORT int mg_grm_weights_device(mg_ctx *c, size_t n_vars, uint32_t n_groups, uint32_t n_samples, const void *d_sites, int haploid, uint32_t maf_ppm, uint32_t min_n,
                                    void *d_q_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_grm_weights(c, n_vars, n_groups, n_samples, d_sites, maf_ppm, min_n, d_q_out));
    if (n_vars) {
        grm_launch_weights(c, n_vars, 0, n_vars, n_groups, n_samples, d_sites, haploid, maf_ppm, min_n, d_q_out, nullptr);
        HIP_TRY(c, hipGetLastError());
    }
    return MG_OK;
}

MG_EXPORT int mg_grm_weights(mg_ctx *c, size_t n_vars, uint32_t n_groups, uint32_t n_samples, const uint64_t *sites, int haploid, uint32_t maf_ppm, uint32_t min_n,
                             int16_t *q_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_grm_weights(c, n_vars, n_groups, n_samples, sites, maf_ppm, min_n, q_out));
    void *d_sites, *d_q;
    TRY(upload(c, c->grm_in[0], sites, 8 * (size_t)n_groups * 3 * n_vars, &d_sites));
    TRY(scratch(c, c->grm_in[1], n_vars ? 8 * n_vars : 1, &d_q));
    TRY(mg_grm_weights_device(c, n_vars, n_groups, n_samples, d_sites, haploid, maf_ppm, min_n, d_q));
    if (n_vars) HIP_TRY(c, hipMemcpyAsync(q_out, d_q, 8 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_grm_begin(mg_ctx *c, uint32_t n_samples, int haploid, uint32_t maf_ppm, uint32_t min_n)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_samples < 1 || n_samples > MG_GRM_MAX_SAMPLES) return fail(c, MG_ERR_ARG, "mg_grm_begin: n_samples is 1..%d", MG_GRM_MAX_SAMPLES);
    if (maf_ppm > 500000) return fail(c, MG_ERR_ARG, "mg_grm_begin: maf_ppm is 0..500000");
    if (min_n < 1) return fail(c, MG_ERR_ARG, "mg_grm_begin: min_n is at least 1");
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a step of the state that goes may still run)
    grm_drop(c);
    const u64 n_pairs = (u64)n_samples * (n_samples + 1) / 2;
    const size_t bytes = 16 * n_pairs + 8; // the sums, the counts, the records that entered
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MG_ERR_NOMEM, "mg_grm_begin: the state of %llu pairs (%zu bytes) does not fit", (unsigned long long)n_pairs, bytes);
    }
    c->grm_state = p;
    c->grm_pairs = n_pairs;
    c->grm_samples = n_samples;
    c->grm_haploid = haploid != 0;
    c->grm_maf_ppm = maf_ppm;
    c->grm_min_n = min_n;
    c->grm_timed = false;
    HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->stream));
    return MG_OK;
}

MG_EXPORT int mg_grm_end(mg_ctx *c)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    grm_drop(c);
    return MG_OK;
}

// The step in pieces of at most `grm_scratch_mb` MiB of byte images (3 bytes per padded sample and record, at least GRM_K records): per piece
// the weights, the expansion, the Gram kernel.  A block of pairs gets as many runs along the records as fill the device, none longer than
// GRM_MAX_RUN; with one run per block the fold needs no atomics.
MG_EXPORT int mg_grm_step_device(mg_ctx *c, size_t n_vars, uint32_t n_groups, const void *d_sites)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_grm_step(c, n_vars, n_groups, d_sites));
    c->grm_ms[0] = c->grm_ms[1] = 0.f;
    c->grm_timed = true;
    c->grm_tm.valid = false;
    c->grm_seen += n_vars;
    if (!n_vars) return MG_OK;
    const u32 n = c->grm_samples, rows = grm_rows(n), blocks = rows / GRM_BLOCK;
    const u64 piece_max = grm_piece_max(rows, (u64)c->grm_scratch_mb << 20); // (the cut into pieces and runs: grm_plan.h)
    long long *d_sum = (long long *)c->grm_state;
    unsigned long long *d_count = (unsigned long long *)c->grm_state + c->grm_pairs, *d_entered = d_count + c->grm_pairs;
    for (u64 v0 = 0; v0 < n_vars; v0 += piece_max) {
        const u64 piece = std::min<u64>(piece_max, n_vars - v0), ld = grm_ld(piece);
        if (c->grm_tm.valid) { // the piece before: its events are about to be used again
            float ms[2];
            TRY(timer_read(c, c->grm_tm, ms));
            c->grm_ms[0] += ms[0];
            c->grm_ms[1] += ms[1];
        }
        void *d_q, *d_img;
        TRY(scratch(c, c->s_grm[0], 8 * piece, &d_q));
        TRY(scratch(c, c->s_grm[1], 3 * (size_t)rows * ld, &d_img));
        TRY(timer_begin(c, c->grm_tm));
        grm_launch_weights(c, n_vars, v0, piece, n_groups, n, d_sites, c->grm_haploid, c->grm_maf_ppm, c->grm_min_n, d_q, d_entered);
        signed char *h = (signed char *)d_img, *l = h + (size_t)rows * ld, *cc = l + (size_t)rows * ld;
        const GrmExpandArgs e{(u64)n_vars, v0, piece, ld, n_groups, n, rows, (const unsigned long long *)d_sites, (const short4 *)d_q, c->grm_haploid, h, l, cc};
        hipLaunchKernelGGL(grm_expand_kernel, dim3((unsigned)((ld / 4 + GRM_TPB - 1) / GRM_TPB), (rows + 63) / 64), dim3(GRM_TPB), 0, c->stream, e);
        HIP_TRY(c, hipGetLastError());
        TRY(timer_mark(c, c->grm_tm, 1));
        uint64_t runs = 0;
        const u64 run = grm_run_plan(ld, blocks, &runs);
        const GrmGramArgs g{ld, run, n, h, l, cc, d_sum, d_count};
        if (runs > 1) hipLaunchKernelGGL(grm_gram_kernel<true>, dim3(blocks, blocks, (unsigned)runs), dim3(64), 0, c->stream, g);
        else hipLaunchKernelGGL(grm_gram_kernel<false>, dim3(blocks, blocks, 1), dim3(64), 0, c->stream, g);
        HIP_TRY(c, hipGetLastError());
        TRY(timer_mark(c, c->grm_tm, 2));
    }
    return MG_OK;
}

MG_EXPORT int mg_grm_step(mg_ctx *c, size_t n_vars, uint32_t n_groups, const uint64_t *sites)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_grm_step(c, n_vars, n_groups, sites));
    void *d_sites;
    TRY(upload(c, c->grm_in[0], sites, 8 * (size_t)n_groups * 3 * n_vars, &d_sites));
    TRY(mg_grm_step_device(c, n_vars, n_groups, d_sites));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_grm_read(mg_ctx *c, int64_t *sum_out, uint64_t *n_out, uint64_t *records_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (!c->grm_state) return fail(c, MG_ERR_STATE, "mg_grm_read: no mg_grm_begin yet");
    if (!sum_out || !n_out || !records_out) return fail(c, MG_ERR_ARG, "NULL argument");
    const char *state = (const char *)c->grm_state;
    TRY(timer_begin(c, c->grm_read_tm));
    HIP_TRY(c, hipMemcpyAsync(sum_out, state, 8 * c->grm_pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(n_out, state + 8 * c->grm_pairs, 8 * c->grm_pairs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&records_out[1], state + 16 * c->grm_pairs, 8, hipMemcpyDeviceToHost, c->stream));
    TRY(timer_mark(c, c->grm_read_tm, 1));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    records_out[0] = c->grm_seen;
    return MG_OK;
}

// device milliseconds (waits for them): ms_out[0] weights + expand and [1] gram of the most recent step, all its pieces; [2] the most
// recent read; 0 where there was none
MG_EXPORT int mg_grm_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = ms_out[1] = ms_out[2] = 0.f; // (also where it fails)
    if (!c->grm_timed && !c->grm_read_tm.valid) return fail(c, MG_ERR_STATE, "no mg_grm_step or mg_grm_read yet");
    float ms[2] = {0.f, 0.f};
    TRY(timer_read(c, c->grm_tm, ms));
    ms_out[0] = c->grm_ms[0] + ms[0];
    ms_out[1] = c->grm_ms[1] + ms[1];
    return timer_read(c, c->grm_read_tm, &ms_out[2]);
}

// ---- principal components of a resident symmetric matrix (pca_kernels.h, pca_plan.h) -----------------------------------------------------
namespace {
enum { PCA_PH_PRODUCT, PCA_PH_ORTH, PCA_PH_RITZ, PCA_PH_OTHER };
void pca_drop(mg_ctx *c)
{
    if (c->pca_g) hipFree(c->pca_g);
    c->pca_g = nullptr;
    c->pca_n = 0;
    c->pca_checked = false;
}
u32 *pca_flag(const mg_ctx *c)
{
    const u64 np = pca_np(c->pca_n);
    return (u32 *)((double *)c->pca_g + np * np);
}
// an event behind what is on the stream; the interval that ends at it belongs to `phase`
int pca_tick(mg_ctx *c, int phase)
{
    if (c->pca_ev_used == c->pca_ev.size()) {
        hipEvent_t e = nullptr;
        HIP_TRY(c, hipEventCreate(&e));
        c->pca_ev.push_back(e);
        c->pca_ev_phase.push_back(PCA_PH_OTHER);
    }
    HIP_TRY(c, hipEventRecord(c->pca_ev[c->pca_ev_used], c->stream));
    c->pca_ev_phase[c->pca_ev_used++] = phase;
    return MG_OK;
}
// after a wait: the intervals so far go to their phases and to the total; the last event becomes the first of what follows
int pca_flush(mg_ctx *c)
{
    for (size_t i = 1; i < c->pca_ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->pca_ev[i - 1], c->pca_ev[i]));
        if (c->pca_ev_phase[i] != PCA_PH_OTHER) c->pca_ms[c->pca_ev_phase[i]] += ms;
        c->pca_ms[3] += ms;
    }
    if (c->pca_ev_used > 1) {
        std::swap(c->pca_ev[0], c->pca_ev[c->pca_ev_used - 1]);
        c->pca_ev_used = 1;
    }
    return MG_OK;
}
template <typename T> int pca_load_device(mg_ctx *c, uint32_t n, const void *d_src, int packed)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (a solve of the matrix that goes has ended; a load of it may still run)
    pca_drop(c);
    const u64 np = pca_np(n);
    const size_t bytes = 8 * np * np + 8; // the matrix and the flag
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MG_ERR_NOMEM, "mg_pca_load: the matrix of %u samples (%zu bytes) does not fit", n, bytes);
    }
    c->pca_g = p;
    c->pca_n = n;
    HIP_TRY(c, hipMemsetAsync(pca_flag(c), 0, 8, c->stream));
    const PcaExpandArgs<T> a{(const T *)d_src, (double *)p, n, (u32)np, packed, pca_flag(c)};
    hipLaunchKernelGGL(pca_expand_kernel<T>, dim3((unsigned)((np * np + PCA_TPB - 1) / PCA_TPB)), dim3(PCA_TPB), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
// waits; the flag of the load, once per load
int pca_check_finite(mg_ctx *c, const char *who)
{
    if (c->pca_checked) return MG_OK;
    u32 bad = 0;
    HIP_TRY(c, hipMemcpyAsync(&bad, pca_flag(c), 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bad) {
        pca_drop(c);
        return fail(c, MG_ERR_ARG, "%s: the matrix holds a value that is not finite (the load is dropped)", who);
    }
    c->pca_checked = true;
    return MG_OK;
}
int check_pca_load(mg_ctx *c, uint32_t n, const void *src)
{
    if (n < 1 || n > MG_PCA_MAX_N) return fail(c, MG_ERR_ARG, "mg_pca_load: n is 1..%d", MG_PCA_MAX_N);
    if (!src) return fail(c, MG_ERR_ARG, "NULL argument");
    return MG_OK;
}
template <typename T> int pca_load_host(mg_ctx *c, uint32_t n, const T *src, int packed)
{
    TRY(check_pca_load(c, n, src));
    const size_t count = packed ? (size_t)n * (n + 1) / 2 : (size_t)n * n;
    void *d_src = nullptr;
    if (hipMalloc(&d_src, sizeof(T) * count) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MG_ERR_NOMEM, "mg_pca_load: the input of %u samples (%zu bytes) does not fit", n, sizeof(T) * count);
    }
    int rc = MG_OK;
    if (hipMemcpyAsync(d_src, src, sizeof(T) * count, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(c, MG_ERR_HIP, "mg_pca_load: the upload failed");
    if (rc == MG_OK) rc = pca_load_device<T>(c, n, d_src, packed);
    if (rc == MG_OK) rc = pca_check_finite(c, "mg_pca_load");
    else (void)hipStreamSynchronize(c->stream);
    hipFree(d_src);
    return rc;
}

struct PcaWork { // a solve's device tables, all inside pca_work
    double *blk[4], *parts, *gparts, *w, *s, *theta, *norm;
    u32 *flags;
};
int pca_launch_gram(mg_ctx *c, const PcaWork &k, const double *a, const double *b, u32 np, u32 m)
{
    const u32 blocks = pca_red_blocks(np);
    hipLaunchKernelGGL(pca_gram_part_kernel, dim3(blocks), dim3(PCA_TPB), 0, c->stream, a, b, np, m, k.gparts);
    hipLaunchKernelGGL(pca_gram_sum_kernel, dim3((m * m + PCA_TPB - 1) / PCA_TPB), dim3(PCA_TPB), 0, c->stream, (const double *)k.gparts, blocks, m * m, k.w);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int pca_launch_update(mg_ctx *c, const double *in, const double *s, u32 np, u32 m, double *out)
{
    hipLaunchKernelGGL(pca_update_kernel, dim3((np + 63) / 64), dim3(PCA_TPB), 0, c->stream, in, s, np, m, out);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
// x -> orthonormal columns in `out`, through `tmp`; collapsed columns of the first pass are replaced by fresh hashed vectors (salt)
int pca_orthonormalise(mg_ctx *c, const PcaWork &k, const double *x, double *tmp, double *out, u32 n, u32 np, u32 m, u64 salt)
{
    TRY(pca_launch_gram(c, k, x, x, np, m));
    hipLaunchKernelGGL(pca_chol_kernel, dim3(1), dim3(PCA_TPB), 0, c->stream, (const double *)k.w, m, k.s, k.flags);
    TRY(pca_launch_update(c, x, k.s, np, m, tmp));
    hipLaunchKernelGGL(pca_fill_kernel, dim3((unsigned)(((u64)np * m + PCA_TPB - 1) / PCA_TPB)), dim3(PCA_TPB), 0, c->stream, tmp, n, np, m, salt, (const u32 *)k.flags);
    TRY(pca_launch_gram(c, k, tmp, tmp, np, m));
    hipLaunchKernelGGL(pca_chol_kernel, dim3(1), dim3(PCA_TPB), 0, c->stream, (const double *)k.w, m, k.s, k.flags);
    TRY(pca_launch_update(c, tmp, k.s, np, m, out));
    return MG_OK;
}
int pca_launch_product(mg_ctx *c, const PcaWork &k, const double *q, double *y, u32 np, u32 m)
{
    u32 chunk = 0;
    const u32 splits = pca_splits(np, &chunk);
    const PcaProductArgs a{(const double *)c->pca_g, q, splits > 1 ? k.parts : y, np, m, chunk};
    const dim3 grid(np / PCA_TILE, splits), block(64 * PCA_WAVES);
    if (m == 32) hipLaunchKernelGGL(pca_product_kernel<2>, grid, block, 0, c->stream, a);
    else if (m == 48) hipLaunchKernelGGL(pca_product_kernel<3>, grid, block, 0, c->stream, a);
    else hipLaunchKernelGGL(pca_product_kernel<4>, grid, block, 0, c->stream, a);
    if (splits > 1) {
        const u64 count = (u64)np * m;
        hipLaunchKernelGGL(pca_sum_parts_kernel, dim3((unsigned)((count + PCA_TPB - 1) / PCA_TPB)), dim3(PCA_TPB), 0, c->stream, (const double *)k.parts, splits, count, y);
    }
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}
int check_pca_solve(mg_ctx *c, uint32_t k, double tol, uint32_t max_iters, const void *values, const void *vectors, const void *resid, const void *scale, const void *info)
{
    if (!values || !vectors || !resid || !scale || !info) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!std::isfinite(tol) || !(tol > 0.0)) return fail(c, MG_ERR_ARG, "mg_pca_solve: tol is finite and above 0");
    if (max_iters == 0) return fail(c, MG_ERR_ARG, "mg_pca_solve: max_iters is at least 1");
    if (!c->pca_g) return fail(c, MG_ERR_STATE, "mg_pca_solve: no mg_pca_load yet");
    const u32 k_max = c->pca_n < MG_PCA_MAX_K ? c->pca_n : MG_PCA_MAX_K;
    if (k < 1 || k > k_max) return fail(c, MG_ERR_ARG, "mg_pca_solve: k is 1..%u for this matrix", k_max);
    return MG_OK;
}
// m == n: the matrix itself goes through the small solver; residuals and the sign rule on the host.  vectors: [k][n]
int pca_solve_small(mg_ctx *c, u32 k, double *values, double *vectors, double *norms, double *scale)
{
    const u32 n = c->pca_n, np = pca_np(n);
    std::vector<double> g((size_t)n * n), a, w(n), v((size_t)n * n);
    HIP_TRY(c, hipMemcpy2DAsync(g.data(), 8 * (size_t)n, c->pca_g, 8 * (size_t)np, 8 * (size_t)n, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    a = g;
    if (pca_jacobi(n, a.data(), w.data(), v.data()) < 0) return fail(c, MG_ERR_LIMIT, "mg_pca_solve: the small eigenproblem did not settle in 64 sweeps");
    double s = 0.0;
    for (u32 j = 0; j < n; ++j) s = std::fabs(w[j]) > s ? std::fabs(w[j]) : s;
    *scale = s > 0.0 ? s : 1.0;
    for (u32 j = 0; j < k; ++j) {
        double sum = 0.0, best = -1.0;
        u32 where = 0;
        for (u32 i = 0; i < n; ++i) {
            double gv = 0.0;
            for (u32 t = 0; t < n; ++t) gv += g[(size_t)i * n + t] * v[(size_t)t * n + j];
            const double d = gv - w[j] * v[(size_t)i * n + j];
            sum += d * d;
            if (std::fabs(v[(size_t)i * n + j]) > best) best = std::fabs(v[(size_t)i * n + j]), where = i;
        }
        const bool flip = v[(size_t)where * n + j] < 0.0;
        values[j] = w[j];
        norms[j] = std::sqrt(sum);
        for (u32 i = 0; i < n; ++i) vectors[(size_t)j * n + i] = flip ? -v[(size_t)i * n + j] : v[(size_t)i * n + j];
    }
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_pca_load_tri_f32_device(mg_ctx *c, uint32_t n, const void *d_tri)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_pca_load(c, n, d_tri));
    return pca_load_device<float>(c, n, d_tri, 1);
}
MG_EXPORT int mg_pca_load_f64_device(mg_ctx *c, uint32_t n, const void *d_full)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_pca_load(c, n, d_full));
    return pca_load_device<double>(c, n, d_full, 0);
}
MG_EXPORT int mg_pca_load_tri_f32(mg_ctx *c, uint32_t n, const float *tri)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    return pca_load_host<float>(c, n, tri, 1);
}
MG_EXPORT int mg_pca_load_f64(mg_ctx *c, uint32_t n, const double *full)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    return pca_load_host<double>(c, n, full, 0);
}
MG_EXPORT int mg_pca_end(mg_ctx *c)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    pca_drop(c);
    return MG_OK;
}

// The solve: products, orthonormalisations and, every PCA_CHECK_EVERY products (and at the last one allowed), a Rayleigh-Ritz step with the
// residual test.  A Rayleigh-Ritz step waits twice -- for H on its way to the host's Jacobi and for the residual norms -- so the call
// returns with everything done; what it put on the stream last are the copies into the outputs.
MG_EXPORT int mg_pca_solve_device(mg_ctx *c, uint32_t k, double tol, uint32_t max_iters, void *d_values_out, void *d_vectors_out, void *d_resid_out, void *d_scale_out,
                                  void *d_info_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_pca_solve(c, k, tol, max_iters, d_values_out, d_vectors_out, d_resid_out, d_scale_out, d_info_out));
    TRY(pca_check_finite(c, "mg_pca_solve"));
    const u32 n = c->pca_n, np = pca_np(n), m = pca_block(n, k);
    c->pca_ms[0] = c->pca_ms[1] = c->pca_ms[2] = c->pca_ms[3] = 0.f;
    c->pca_timed = false;
    c->pca_ev_used = 0;
    TRY(pca_tick(c, PCA_PH_OTHER));
    std::vector<double> values(k), norms(k), resid(k);
    double scale = 1.0;
    u32 products = 0;
    if (m == n) {
        std::vector<double> vectors((size_t)k * n);
        TRY(pca_solve_small(c, k, values.data(), vectors.data(), norms.data(), &scale));
        HIP_TRY(c, hipMemcpyAsync(d_vectors_out, vectors.data(), 8 * (size_t)k * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else {
        const u64 blk = (u64)np * m, mm = (u64)m * m;
        u32 chunk = 0;
        const u32 splits = pca_splits(np, &chunk), red = pca_red_blocks(np);
        const u64 doubles = 4 * blk + (splits > 1 ? splits * blk : 0) + red * mm + 2 * mm + 2 * m;
        void *base;
        TRY(scratch(c, c->pca_work, 8 * doubles + 4 * m, &base));
        PcaWork wk;
        double *p = (double *)base;
        for (double *&b : wk.blk) b = p, p += blk;
        wk.parts = p, p += splits > 1 ? splits * blk : 0;
        wk.gparts = p, p += red * mm;
        wk.w = p, p += mm;
        wk.s = p, p += mm;
        wk.theta = p, p += m;
        wk.norm = p, p += m;
        wk.flags = (u32 *)p;
        double *q = wk.blk[0], *y = wk.blk[1], *t1 = wk.blk[2], *t2 = wk.blk[3];
        u64 salt = 0;
        hipLaunchKernelGGL(pca_fill_kernel, dim3((unsigned)((blk + PCA_TPB - 1) / PCA_TPB)), dim3(PCA_TPB), 0, c->stream, y, n, np, m, salt++, (const u32 *)nullptr);
        TRY(pca_orthonormalise(c, wk, y, t1, q, n, np, m, salt++));
        TRY(pca_tick(c, PCA_PH_ORTH));
        std::vector<double> h(mm), theta(m), s(mm), all_norms(m);
        for (;;) {
            TRY(pca_launch_product(c, wk, q, y, np, m));
            ++products;
            TRY(pca_tick(c, PCA_PH_PRODUCT));
            if (products % PCA_CHECK_EVERY == 0 || products == max_iters) {
                TRY(pca_launch_gram(c, wk, q, y, np, m));
                HIP_TRY(c, hipMemcpyAsync(h.data(), wk.w, 8 * mm, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                for (u32 i = 0; i < m; ++i) // H = Q^T G Q is symmetric up to rounding: the small solver gets the mean of the two halves
                    for (u32 j = i + 1; j < m; ++j) h[(size_t)i * m + j] = 0.5 * (h[(size_t)i * m + j] + h[(size_t)j * m + i]);
                if (pca_jacobi(m, h.data(), theta.data(), s.data()) < 0) return fail(c, MG_ERR_LIMIT, "mg_pca_solve: the small eigenproblem did not settle in 64 sweeps");
                HIP_TRY(c, hipMemcpyAsync(wk.s, s.data(), 8 * mm, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(c, hipMemcpyAsync(wk.theta, theta.data(), 8 * (size_t)m, hipMemcpyHostToDevice, c->stream));
                TRY(pca_launch_update(c, q, wk.s, np, m, t1));
                TRY(pca_launch_update(c, y, wk.s, np, m, t2));
                hipLaunchKernelGGL(pca_resid_kernel, dim3(m), dim3(PCA_TPB), 0, c->stream, (const double *)t1, (const double *)t2, (const double *)wk.theta, np, m, wk.norm);
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipMemcpyAsync(all_norms.data(), wk.norm, 8 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
                TRY(pca_tick(c, PCA_PH_RITZ));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                TRY(pca_flush(c));
                std::swap(q, t1);
                std::swap(y, t2);
                double big = 0.0;
                for (u32 j = 0; j < m; ++j) big = std::fabs(theta[j]) > big ? std::fabs(theta[j]) : big;
                scale = big > 0.0 ? big : 1.0;
                u32 done = 0;
                for (u32 j = 0; j < k; ++j) done += all_norms[j] / scale <= tol;
                if (done == k || products == max_iters) break;
            }
            TRY(pca_orthonormalise(c, wk, y, t1, q, n, np, m, salt++));
            TRY(pca_tick(c, PCA_PH_ORTH));
        }
        for (u32 j = 0; j < k; ++j) values[j] = theta[j], norms[j] = all_norms[j];
        hipLaunchKernelGGL(pca_emit_kernel, dim3(k), dim3(PCA_TPB), 0, c->stream, (const double *)q, n, m, (double *)d_vectors_out);
        HIP_TRY(c, hipGetLastError());
    }
    u32 info[3] = {products, 0, m};
    for (u32 j = 0; j < k; ++j) {
        resid[j] = norms[j] / scale;
        info[1] += resid[j] <= tol;
    }
    HIP_TRY(c, hipMemcpyAsync(d_values_out, values.data(), 8 * (size_t)k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_resid_out, resid.data(), 8 * (size_t)k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_scale_out, &scale, 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_info_out, info, sizeof info, hipMemcpyHostToDevice, c->stream));
    TRY(pca_tick(c, PCA_PH_OTHER));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    TRY(pca_flush(c));
    c->pca_timed = true;
    return MG_OK;
}

MG_EXPORT int mg_pca_solve(mg_ctx *c, uint32_t k, double tol, uint32_t max_iters, double *values_out, double *vectors_out, double *resid_out, double *scale_out,
                           uint32_t *info_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_pca_solve(c, k, tol, max_iters, values_out, vectors_out, resid_out, scale_out, info_out));
    const size_t n = c->pca_n, small = 8 * (2 * (size_t)k + 1) + 16;
    void *d_vec, *d_small;
    TRY(scratch(c, c->pca_io[0], 8 * k * n, &d_vec));
    TRY(scratch(c, c->pca_io[1], small, &d_small));
    double *d_values = (double *)d_small, *d_resid = d_values + k, *d_scale = d_resid + k;
    TRY(mg_pca_solve_device(c, k, tol, max_iters, d_values, d_vec, d_resid, d_scale, d_scale + 1));
    HIP_TRY(c, hipMemcpyAsync(vectors_out, d_vec, 8 * k * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(values_out, d_values, 8 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(resid_out, d_resid, 8 * (size_t)k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scale_out, d_scale, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(info_out, d_scale + 1, 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds of the most recent solve: products, orthonormalisation, Rayleigh-Ritz (the host's part of it included: the device
// waits for the small solver), total
MG_EXPORT int mg_pca_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    for (int i = 0; i < 4; ++i) ms_out[i] = 0.f; // (also where it fails)
    if (!c->pca_timed) return fail(c, MG_ERR_STATE, "no mg_pca_solve yet");
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 4; ++i) ms_out[i] = c->pca_ms[i];
    return MG_OK;
}

// ---- allele priors re-estimated from the planes of a batch (cohort_prior_kernels.h) ------------------------------------------------------
namespace {
int check_cohort_prior(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *cov, const void *freq, const void *var_allele_off, uint32_t iters, double weight,
                       const void *freq_out, const void *n_informative, const void *gt1, const void *gt2, const void *gq, const void *status, const void *probs,
                       const void *var_gt_off)
{
    if (n_planes < 1 || n_planes > 64) return fail(c, MG_ERR_ARG, "mg_genotype_cohort takes 1..64 planes");
    if (iters > 64) return fail(c, MG_ERR_ARG, "mg_genotype_cohort takes at most 64 iterations");
    if (!std::isfinite(weight) || weight < 0) return fail(c, MG_ERR_ARG, "mg_genotype_cohort takes a finite weight >= 0");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_genotype_cohort: more than 2^32 - 1 records in one call");
    if (n_vars && (!cov || !freq || !var_allele_off || !freq_out || !n_informative || !gt1 || !gt2 || !gq || !status)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (probs && !var_gt_off) return fail(c, MG_ERR_ARG, "probs needs var_gt_off");
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_genotype_cohort_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_freq, const void *d_var_allele_off, float error_rate,
                                        int max_cov, int haploid, uint32_t iters, double weight, void *d_freq_out, void *d_n_informative, void *d_gt1, void *d_gt2,
                                        void *d_gq, void *d_status, void *d_probs, const void *d_var_gt_off)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_cohort_prior(c, n_vars, n_planes, d_cov, d_freq, d_var_allele_off, iters, weight, d_freq_out, d_n_informative, d_gt1, d_gt2, d_gq, d_status, d_probs,
                           d_var_gt_off));
    GenoParams p;
    if (n_vars) TRY(fill_geno_params(c, error_rate, max_cov, haploid, &p)); // (may synchronise: before the timer starts)
    TRY(timer_begin(c, c->tm[TM_PRIOR]));
    if (n_vars) {
        u32 seg_log2 = 0;
        while ((1u << seg_log2) < n_planes) ++seg_log2;
        const u32 run = std::max<u32>(PRIOR_TPB >> seg_log2, PRIOR_MIN_RUN); // a multiple of the 256 >> seg_log2 records four waves hold at a time
        const PriorArgs a{(u64)n_vars, n_planes, seg_log2, run, iters, weight, (const u32 *)d_cov, (const float *)d_freq, (const u32 *)d_var_allele_off,
                          (float *)d_freq_out, (u32 *)d_n_informative, (i32 *)d_gt1, (i32 *)d_gt2, (i32 *)d_gq, (u8 *)d_status, (double *)d_probs,
                          (const u64 *)d_var_gt_off};
        hipLaunchKernelGGL(cohort_prior_kernel, dim3((unsigned)((n_vars + run - 1) / run)), dim3(PRIOR_TPB), 0, c->stream, a, p);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_PRIOR], 1);
}

MG_EXPORT int mg_genotype_cohort(mg_ctx *c, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off, float error_rate,
                                 int max_cov, int haploid, uint32_t iters, double weight, float *freq_out, uint32_t *n_informative, int32_t *gt1, int32_t *gt2,
                                 int32_t *gq, uint8_t *status, double *probs, const uint64_t *var_gt_off)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_cohort_prior(c, n_vars, n_planes, cov, freq, var_allele_off, iters, weight, freq_out, n_informative, gt1, gt2, gq, status, probs, var_gt_off));
    const size_t na = n_vars ? var_allele_off[n_vars] : 0, ng = probs && n_vars ? var_gt_off[n_vars] : 0, cells = (size_t)n_planes * n_vars;
    void *d_cov = nullptr, *d_freq = nullptr, *d_off = nullptr, *d_fo = nullptr, *d_ni = nullptr, *d_g1 = nullptr, *d_g2 = nullptr, *d_gq = nullptr, *d_st = nullptr,
         *d_pr = nullptr, *d_go = nullptr;
    if (n_vars) {
        TRY(upload(c, c->stage[ST_COV], cov, 4 * (size_t)n_planes * na, &d_cov));
        TRY(upload(c, c->stage[ST_FREQ], freq, 4 * na, &d_freq));
        TRY(upload(c, c->stage[ST_VAR_ALLELE_OFF], var_allele_off, 4 * (n_vars + 1), &d_off));
        TRY(scratch(c, c->stage[ST_FREQ_OUT], 4 * (na ? na : 1), &d_fo));
        TRY(scratch(c, c->stage[ST_NINF], 4 * n_vars, &d_ni));
        TRY(scratch(c, c->stage[ST_GT1], 4 * cells, &d_g1));
        TRY(scratch(c, c->stage[ST_GT2], 4 * cells, &d_g2));
        TRY(scratch(c, c->stage[ST_GQ], 4 * cells, &d_gq));
        TRY(scratch(c, c->stage[ST_STATUS], cells, &d_st));
        if (probs) {
            TRY(scratch(c, c->stage[ST_PROBS], 8 * ((size_t)n_planes * ng ? (size_t)n_planes * ng : 1), &d_pr));
            TRY(upload(c, c->stage[ST_VAR_GT_OFF], var_gt_off, 8 * (n_vars + 1), &d_go));
        }
    }
    TRY(mg_genotype_cohort_device(c, n_vars, n_planes, d_cov, d_freq, d_off, error_rate, max_cov, haploid, iters, weight, d_fo, d_ni, d_g1, d_g2, d_gq, d_st, d_pr, d_go));
    if (!n_vars) return MG_OK;
    if (na) HIP_TRY(c, hipMemcpyAsync(freq_out, d_fo, 4 * na, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(n_informative, d_ni, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gt1, d_g1, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gt2, d_g2, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gq, d_gq, 4 * cells, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, d_st, cells, hipMemcpyDeviceToHost, c->stream));
    if (probs && ng) HIP_TRY(c, hipMemcpyAsync(probs, d_pr, 8 * (size_t)n_planes * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // cells of the records the entry does not re-estimate that took an ln(n) from the device's log(double): again on the host, with libm, as in
    // mg_genotype (a re-estimated record keeps the device's values: reaching MG_LN_TABLE with at most 8 alleles takes a max_cov of 8192)
    for (size_t v = 0; v < n_vars; ++v) {
        const uint32_t a0 = var_allele_off[v], A = var_allele_off[v + 1] - a0;
        if (iters > 0 && A >= 2 && A <= MG_PRIOR_MAX_ALLELES) continue;
        for (size_t pl = 0; pl < n_planes; ++pl) {
            const size_t cell = pl * n_vars + v;
            if (status[cell] != 0) continue;
            const uint32_t *cv = cov + pl * na + a0;
            int isum = 0;
            for (uint32_t al = 0; al < A; ++al) isum += (int)cv[al];
            if (isum < MG_LN_TABLE) continue;
            host_genotype_one(cv, freq + a0, (int)A, (u32)isum, error_rate, haploid, gt1 + cell, gt2 + cell, gq + cell, probs ? probs + pl * ng + var_gt_off[v] : nullptr);
        }
    }
    return MG_OK;
}

// device milliseconds (waits for them) of the most recent mg_genotype_cohort*
MG_EXPORT int mg_cohort_prior_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = 0.f; // (also where it fails)
    if (!c->tm[TM_PRIOR].valid) return fail(c, MG_ERR_STATE, "no mg_genotype_cohort yet");
    return timer_read(c, c->tm[TM_PRIOR], ms_out);
}

// ---- the estimate alone, for any number of planes (cohort_prior_wide_kernel) ---------------------------------------------------------------
namespace {
int check_estimate_priors(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *cov, const void *freq, const void *var_allele_off, uint32_t iters, double weight,
                          const void *freq_out, const void *n_informative)
{
    if (n_planes < 1 || n_planes > MG_PRIOR_WIDE_MAX_PLANES) return fail(c, MG_ERR_ARG, "mg_estimate_priors takes 1..16384 planes");
    if (iters > 64) return fail(c, MG_ERR_ARG, "mg_estimate_priors takes at most 64 iterations");
    if (!std::isfinite(weight) || weight < 0) return fail(c, MG_ERR_ARG, "mg_estimate_priors takes a finite weight >= 0");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_estimate_priors: more than 2^32 - 1 records in one call");
    if (n_vars && (!cov || !freq || !var_allele_off || !freq_out || !n_informative)) return fail(c, MG_ERR_ARG, "NULL argument");
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_estimate_priors_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_freq, const void *d_var_allele_off, float error_rate,
                                        int max_cov, int haploid, uint32_t iters, double weight, void *d_freq_out, void *d_n_informative)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_estimate_priors(c, n_vars, n_planes, d_cov, d_freq, d_var_allele_off, iters, weight, d_freq_out, d_n_informative));
    GenoParams p;
    if (n_vars) TRY(fill_geno_params(c, error_rate, max_cov, haploid, &p)); // (may synchronise: before the timer starts)
    TRY(timer_begin(c, c->tm[TM_ESTIMATE]));
    if (n_vars) {
        // up to 64 planes: mg_genotype_cohort's segment widths and run; beyond: chunks of 64 planes at width 64, a run of PRIOR_WIDE_RUN
        const u32 n_chunks = (n_planes + 63) / 64;
        u32 seg_log2 = 0;
        while ((1u << seg_log2) < std::min<u32>(n_planes, 64)) ++seg_log2;
        const u32 run = n_chunks > 1 ? PRIOR_WIDE_RUN : std::max<u32>(PRIOR_TPB >> seg_log2, PRIOR_MIN_RUN);
        static_assert(PRIOR_WIDE_RUN % 4 == 0 && PRIOR_WIDE_RUN <= PRIOR_TPB, "four waves, a record each at a time");
        const PriorWideArgs a{(u64)n_vars, n_planes, seg_log2, run, iters, n_chunks, weight, (const u32 *)d_cov, (const float *)d_freq, (const u32 *)d_var_allele_off,
                              (float *)d_freq_out, (u32 *)d_n_informative};
        hipLaunchKernelGGL(cohort_prior_wide_kernel, dim3((unsigned)((n_vars + run - 1) / run)), dim3(PRIOR_TPB), 0, c->stream, a, p);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_ESTIMATE], 1);
}

MG_EXPORT int mg_estimate_priors(mg_ctx *c, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off, float error_rate,
                                 int max_cov, int haploid, uint32_t iters, double weight, float *freq_out, uint32_t *n_informative)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_estimate_priors(c, n_vars, n_planes, cov, freq, var_allele_off, iters, weight, freq_out, n_informative));
    const size_t na = n_vars ? var_allele_off[n_vars] : 0;
    void *d_cov = nullptr, *d_freq = nullptr, *d_off = nullptr, *d_fo = nullptr, *d_ni = nullptr;
    if (n_vars) {
        TRY(upload(c, c->stage[ST_COV], cov, 4 * (size_t)n_planes * na, &d_cov));
        TRY(upload(c, c->stage[ST_FREQ], freq, 4 * na, &d_freq));
        TRY(upload(c, c->stage[ST_VAR_ALLELE_OFF], var_allele_off, 4 * (n_vars + 1), &d_off));
        TRY(scratch(c, c->stage[ST_FREQ_OUT], 4 * (na ? na : 1), &d_fo));
        TRY(scratch(c, c->stage[ST_NINF], 4 * n_vars, &d_ni));
    }
    TRY(mg_estimate_priors_device(c, n_vars, n_planes, d_cov, d_freq, d_off, error_rate, max_cov, haploid, iters, weight, d_fo, d_ni));
    if (!n_vars) return MG_OK;
    if (na) HIP_TRY(c, hipMemcpyAsync(freq_out, d_fo, 4 * na, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(n_informative, d_ni, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them) of the most recent mg_estimate_priors*
MG_EXPORT int mg_estimate_priors_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = 0.f; // (also where it fails)
    if (!c->tm[TM_ESTIMATE].valid) return fail(c, MG_ERR_STATE, "no mg_estimate_priors yet");
    return timer_read(c, c->tm[TM_ESTIMATE], ms_out);
}

// ---- Phred-scaled likelihoods from the coverages, prior-free (pl_kernels.h) ------------------------------------------------------------------
namespace {
int check_phred(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *cov, const void *var_allele_off, const void *var_gt_off, int32_t cap, const void *pl_out)
{
    if (n_planes < 1 || n_planes > 64) return fail(c, MG_ERR_ARG, "mg_phred_likelihoods takes 1..64 planes");
    if (cap < 1) return fail(c, MG_ERR_ARG, "mg_phred_likelihoods takes a cap >= 1");
    if (n_vars >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_phred_likelihoods: more than 2^32 - 1 records in one call");
    if (n_vars && (!cov || !var_allele_off || !var_gt_off || !pl_out)) return fail(c, MG_ERR_ARG, "NULL argument");
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_phred_likelihoods_device(mg_ctx *c, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_var_allele_off, const void *d_var_gt_off,
                                          float error_rate, int max_cov, int haploid, int32_t cap, void *d_pl_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    TRY(check_phred(c, n_vars, n_planes, d_cov, d_var_allele_off, d_var_gt_off, cap, d_pl_out));
    GenoParams p;
    if (n_vars) TRY(fill_geno_params(c, error_rate, max_cov, haploid, &p)); // (may synchronise: before the timer starts)
    TRY(timer_begin(c, c->tm[TM_PL]));
    if (n_vars) {
        const PlArgs a{(u64)n_vars, (const u32 *)d_cov, (const u32 *)d_var_allele_off, (const u64 *)d_var_gt_off, cap, (i32 *)d_pl_out};
        hipLaunchKernelGGL(pl_kernel, dim3((unsigned)((n_vars + PL_TPB - 1) / PL_TPB), n_planes), dim3(PL_TPB), 0, c->stream, a, p);
        HIP_TRY(c, hipGetLastError());
    }
    return timer_mark(c, c->tm[TM_PL], 1);
}

MG_EXPORT int mg_phred_likelihoods(mg_ctx *c, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const uint32_t *var_allele_off, const uint64_t *var_gt_off,
                                   float error_rate, int max_cov, int haploid, int32_t cap, int32_t *pl_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    TRY(check_phred(c, n_vars, n_planes, cov, var_allele_off, var_gt_off, cap, pl_out));
    const size_t na = n_vars ? var_allele_off[n_vars] : 0, ng = n_vars ? var_gt_off[n_vars] : 0;
    void *d_cov = nullptr, *d_vao = nullptr, *d_vgo = nullptr, *d_pl = nullptr;
    for (size_t v = 0; v < n_vars; ++v) { // (the kernel leaves such a record alone; here the offsets can be read, and nothing is written)
        const uint64_t A = var_allele_off[v + 1] - var_allele_off[v];
        if (var_allele_off[v + 1] < var_allele_off[v] || var_gt_off[v + 1] - var_gt_off[v] != (haploid ? A : A * (A + 1) / 2))
            return fail(c, MG_ERR_ARG, "mg_phred_likelihoods: record %zu's slice of var_gt_off is not its number of genotypes", v);
    }
    if (n_vars) {
        TRY(upload(c, c->stage[ST_COV], cov, 4 * (size_t)n_planes * na, &d_cov));
        TRY(upload(c, c->stage[ST_VAR_ALLELE_OFF], var_allele_off, 4 * (n_vars + 1), &d_vao));
        TRY(upload(c, c->stage[ST_VAR_GT_OFF], var_gt_off, 8 * (n_vars + 1), &d_vgo));
        TRY(scratch(c, c->stage[ST_PL], 4 * ((size_t)n_planes * ng ? (size_t)n_planes * ng : 1), &d_pl));
    }
    TRY(mg_phred_likelihoods_device(c, n_vars, n_planes, d_cov, d_vao, d_vgo, error_rate, max_cov, haploid, cap, d_pl));
    if (n_vars && ng) HIP_TRY(c, hipMemcpyAsync(pl_out, d_pl, 4 * (size_t)n_planes * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// device milliseconds (waits for them) of the most recent mg_phred_likelihoods*
MG_EXPORT int mg_pl_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    ms_out[0] = 0.f; // (also where it fails)
    if (!c->tm[TM_PL].valid) return fail(c, MG_ERR_STATE, "no mg_phred_likelihoods yet");
    return timer_read(c, c->tm[TM_PL], ms_out);
}

MG_EXPORT int mg_encode_calls_bcf_device(mg_ctx *c, const mg_cells *cells, const mg_bcf_keys *keys, void *d_out, size_t out_cap, void *d_row_off_out, uint64_t *bytes_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !cells || !keys) return MG_ERR_ARG;
    const mg_cells &x = *cells;
    const mg_bcf_keys &k = *keys;
    const bool gp = has_gp(x), with_pl = has_pl(x);
    TRY(check_cells(c, "mg_encode_calls_bcf", x, true, true));
    if (k.gt < 0 || k.gq < 0 || (x.cov && k.cov < 0) || (gp && k.gp < 0) || (with_pl && k.pl < 0)) return fail(c, MG_ERR_ARG, "mg_encode_calls_bcf: a dictionary index is >= 0");
    const BcfArgs a{(u64)x.n_vars, x.n_planes, x.haploid, (const i32 *)x.gt1, (const i32 *)x.gt2, (const i32 *)x.gq, (const u32 *)x.cov, (const u32 *)x.var_allele_off,
                    x.use_mask, x.min_gq, k.gt, k.gq, k.cov, (const double *)x.probs, (const u64 *)x.var_gt_off, (const u8 *)x.status, k.gp, (const i32 *)x.pl, k.pl};
    const auto len_kernel = with_pl ? (gp ? bcf_len_kernel<true, true> : bcf_len_kernel<false, true>) : gp ? bcf_len_kernel<true> : bcf_len_kernel<false>;
    const auto write_kernel = with_pl ? (gp ? bcf_write_kernel<true, true> : bcf_write_kernel<false, true>) : gp ? bcf_write_kernel<true> : bcf_write_kernel<false>;
    void *d_types = nullptr; // the records' type codes (three, with PL four): what the length pass found, for the write pass
    return encode_rows(
        c, TM_BCF, "mg_encode_calls_bcf", x.n_vars, d_out, out_cap, d_row_off_out, bytes_out,
        [&](u32 *len, unsigned long long *meta) -> int {
            TRY(scratch(c, c->s_enc[TM_BCF][ES_TYPES], (with_pl ? 4 : 3) * x.n_vars, &d_types));
            hipLaunchKernelGGL(len_kernel, fmt_len_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, len, (unsigned char *)d_types, meta);
            return MG_OK;
        },
        [&](const unsigned long long *row_off) {
            hipLaunchKernelGGL(write_kernel, fmt_write_grid(x.n_vars), dim3(FMT_TPB), 0, c->stream, a, (const unsigned char *)d_types, row_off, (char *)d_out, (u64)out_cap);
        });
}

MG_EXPORT int mg_encode_calls_bcf(mg_ctx *c, const mg_cells *cells, const mg_bcf_keys *keys, uint8_t *out, size_t out_cap, uint64_t *row_off_out, uint64_t *bytes_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || !cells || !keys) return MG_ERR_ARG;
    const mg_cells &x = *cells;
    TRY(check_cells(c, "mg_encode_calls_bcf", x, true, true));
    TRY(check_rows_out(c, out, out_cap, row_off_out, bytes_out));
    mg_cells d;
    void *d_out, *d_off;
    TRY(stage_cells(c, x, &d, true, true));
    TRY(stage_rows(c, x.n_vars, out_cap, &d_out, &d_off));
    const int rc = mg_encode_calls_bcf_device(c, &d, keys, d_out, out_cap, d_off, bytes_out);
    return fetch_rows(c, rc, x.n_vars, d_out, d_off, out, out_cap, row_off_out, bytes_out);
}

// device milliseconds of the most recent mg_encode_calls_bcf* (rows_stats)
MG_EXPORT int mg_bcf_stats(mg_ctx *c, float *ms_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out) return MG_ERR_ARG;
    return rows_stats(c, TM_BCF, "mg_encode_calls_bcf", ms_out);
}

// timing and counts of the most recent mg_cover_blocks_device (waits for it)
MG_EXPORT int mg_blocks_stats(mg_ctx *c, float *ms_out, uint64_t *counts_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c || !ms_out || !counts_out) return MG_ERR_ARG;
    if (!c->tm[TM_BLOCKS].valid) return fail(c, MG_ERR_STATE, "no mg_cover_blocks_device yet");
    TRY(timer_read(c, c->tm[TM_BLOCKS], ms_out));
    unsigned long long h[8];
    HIP_TRY(c, hipMemcpy(h, c->d_gen_count, 64, hipMemcpyDeviceToHost));
    counts_out[0] = h[0];
    counts_out[1] = h[2];
    counts_out[2] = h[3];
    counts_out[3] = h[4];
    return MG_OK;
}

namespace {
// the host forms' panel: every block its own "sequence" (blk_ref_base / blk_ref_len as the caller gives them)
// *out: x on the device (a non-NULL sp_off: the sparse genotypes, and `gt` stays behind); *d_var_block: the block of every record
int upload_blocks(mg_ctx *c, const mg_blocks_host &x, mg_panel_dev *out, void **d_blk_var_off, void **d_var_block, void **d_n_blocks)
{
    if (!x.blk_ref_base || !x.blk_ref_len || !x.blk_var_off || !x.pos || !x.ref_size || !x.min_size || !x.present || !x.var_allele_off || !x.allele_off || !x.pool ||
        !x.canon || (x.n_samples && !x.gt && !x.sp_off) || (x.sp_off && (!x.sp_sample || !x.sp_gt)))
        return fail(c, MG_ERR_ARG, "NULL argument");
    const size_t n_blocks = x.n_blocks, n_vars = x.n_vars;
    if (x.sp_off)
        for (size_t v = 0; v < n_vars; ++v) {
            if (x.sp_off[v + 1] < x.sp_off[v] || x.sp_off[v + 1] - x.sp_off[v] > x.n_samples) return fail(c, MG_ERR_ARG, "sparse genotype offsets of record %zu", v);
            for (u32 e = x.sp_off[v]; e < x.sp_off[v + 1]; ++e)
                if (x.sp_sample[e] >= x.n_samples || (e > x.sp_off[v] && x.sp_sample[e] <= x.sp_sample[e - 1]))
                    return fail(c, MG_ERR_ARG, "sparse genotypes of record %zu: samples must ascend below n_samples", v);
        }
    if (!c->d_ref) return fail(c, MG_ERR_STATE, "mg_reference_upload first");
    if (x.blk_var_off[n_blocks] != n_vars) return fail(c, MG_ERR_ARG, "block offsets do not close");
    const size_t na = x.var_allele_off[n_vars];
    if (x.allele_off[na] > x.pool_len) return fail(c, MG_ERR_ARG, "allele offsets exceed the pool");
    std::vector<u32> var_block(n_vars);
    for (size_t b = 0; b < n_blocks; ++b) {
        if (x.blk_ref_base[b] + x.blk_ref_len[b] > c->ref_len) return fail(c, MG_ERR_ARG, "block %zu lies outside the uploaded reference", b);
        for (u32 v = x.blk_var_off[b]; v < x.blk_var_off[b + 1]; ++v) var_block[v] = (u32)b;
    }
    auto up = [&](Scratch &s, const void *host, size_t bytes, auto *dev) -> int {
        void *p = nullptr;
        TRY(upload(c, s, host, bytes, &p));
        *dev = static_cast<std::remove_reference_t<decltype(*dev)>>(p);
        return MG_OK;
    };
    mg_panel_dev p{};
    p.n_vars = n_vars;
    p.n_contigs = (uint32_t)n_blocks;
    p.n_samples = x.n_samples;
    p.pool_bytes = x.pool_len;
    p.sp_default = x.sp_default;
    const u32 *d_bo;
    TRY(up(c->s_misc[0], x.blk_ref_base, 8 * n_blocks, &p.contig_base));
    TRY(up(c->s_misc[1], x.blk_ref_len, 4 * n_blocks, &p.contig_len));
    TRY(up(c->s_misc[2], x.blk_var_off, 4 * (n_blocks + 1), &d_bo));
    TRY(up(c->s_misc[3], var_block.data(), 4 * n_vars, &p.contig_id));
    TRY(up(c->s_misc[4], x.pos, 4 * n_vars, &p.pos));
    TRY(up(c->s_misc[5], x.ref_size, 4 * n_vars, &p.ref_size));
    TRY(up(c->s_misc[6], x.min_size, 4 * n_vars, &p.min_size));
    TRY(up(c->s_misc[7], x.present, n_vars, &p.present));
    TRY(up(c->s_rows, x.var_allele_off, 4 * (n_vars + 1), &p.var_allele_off));
    TRY(up(c->s_aux, x.allele_off, 4 * (na + 1), &p.allele_off));
    TRY(up(c->s_open[0], x.pool, x.pool_len, &p.pool));
    TRY(up(c->s_open[1], x.canon, na, &p.canon));
    if (x.sp_off) {
        const size_t ne = x.sp_off[n_vars];
        TRY(up(c->s_open[2], x.sp_off, 4 * (n_vars + 1), &p.sp_off));
        TRY(up(c->s_hit[0], x.sp_sample, 4 * ne, &p.sp_sample));
        TRY(up(c->s_hit[1], x.sp_gt, 2 * ne, &p.sp_gt));
    } else
        TRY(up(c->s_open[2], x.gt, 2 * n_vars * x.n_samples, &p.gt));
    if (!c->d_gen_count) HIP_TRY(c, hipMalloc(&c->d_gen_count, 64));
    const unsigned long long nb = n_blocks;
    HIP_TRY(c, hipMemcpyAsync(c->d_gen_count + 1, &nb, 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (`nb` and `var_block` live on this frame)
    *out = p;
    *d_blk_var_off = (void *)d_bo;
    *d_var_block = (void *)p.contig_id;
    *d_n_blocks = c->d_gen_count + 1;
    return MG_OK;
}

int cover_blocks_host(mg_ctx *c, const mg_blocks_host &x, int haploid, uint32_t *cov_out, uint8_t *overflow_out, bool all_planes)
{
    const DeviceGuard on_device(c, KEEP);
    if (x.n_vars == 0) return MG_OK;
    if (!cov_out || !overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    mg_panel_dev p{};
    void *d_bo, *d_vb, *d_nb;
    TRY(upload_blocks(c, x, &p, &d_bo, &d_vb, &d_nb));
    const size_t slots = x.var_allele_off[x.n_vars], na = slots * (all_planes ? c->coh_planes : 1);
    void *d_cov, *d_ovf;
    TRY(scratch(c, c->s_out, 4 * na, &d_cov));
    TRY(scratch(c, c->s_irr, x.n_vars, &d_ovf));
    if (all_planes) TRY(cover_cohort(c, &p, d_bo, d_vb, d_nb, haploid, d_cov, d_ovf, slots));
    else TRY(mg_cover_blocks_device(c, &p, d_bo, d_vb, d_nb, haploid, d_cov, d_ovf));
    HIP_TRY(c, hipMemcpyAsync(cov_out, d_cov, 4 * na, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(overflow_out, d_ovf, x.n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_cover_blocks(mg_ctx *c, const mg_blocks_host *x, int haploid, uint32_t *cov_out, uint8_t *overflow_out)
{
    if (!c || !x) return MG_ERR_ARG;
    return cover_blocks_host(c, *x, haploid, cov_out, overflow_out, false);
}
// the batch goes up once and is covered for every plane of a context in cohort mode: cov_out is [n_planes][slots]
MG_EXPORT int mg_cover_blocks_cohort(mg_ctx *c, const mg_blocks_host *x, int haploid, uint32_t *cov_out, uint8_t *overflow_out)
{
    if (!c || !x) return MG_ERR_ARG;
    if (!c->coh_planes) return fail(c, MG_ERR_STATE, "mg_cover_blocks_cohort: not in cohort mode (mg_cohort_begin first)");
    return cover_blocks_host(c, *x, haploid, cov_out, overflow_out, true);
}

// index time: VB::extract_kmers + add_kmers_to_bf (main.cpp:349-350, 122-144) for every block of a resident panel.  Synchronises
// once on eight bytes: the exact map is sized from the counting pass before the insert pass runs.
MG_EXPORT int mg_index_blocks_device(mg_ctx *c, const mg_panel_dev *p, const void *d_blk_var_off, const void *d_var_block, const void *d_n_blocks, int haploid,
                                     void *d_overflow_out)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    TRY(check_panel(c, p, true));
    if (p->n_vars == 0) return MG_OK;
    if (!d_blk_var_off || !d_n_blocks || !d_overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (c->bf[MG_BF_ALT].mode) return fail(c, MG_ERR_STATE, "mg_index_blocks after mg_bf_finalize");
    const u64 n = p->n_vars;
    if (c->map.rows_total + n >= 0xFFFFFFFFULL) return fail(c, MG_ERR_LIMIT, "exact map: more than 2^32-1 insertion rows");
    TRY(map_reserve(c, n)); // the lone records' REF keys take insertion rows rows_total + v; may grow and re-hash the table: before the kernels, never under one
    BlocksRun R{};
    TRY(blocks_setup(c, p, (const u32 *)d_blk_var_off, (const u32 *)d_var_block, (const unsigned long long *)d_n_blocks, haploid, &R));
    c->gate_dirty = true;
    HIP_TRY(c, hipMemsetAsync(d_overflow_out, 0, n, c->stream));
    HIP_TRY(c, hipMemsetAsync(R.fb_flag, 0, n, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_gen_count, 0, 64, c->stream));
    // tier 1: lone and short records are inserted at once; everything else is listed
    const int tiles = lone_tiles_for(c, n);
    hipLaunchKernelGGL(panel_lone_index_kernel, dim3(lone_grid(n, tiles)), dim3(TPB), 0, c->stream, R.P, n, R.B.blk_var_off, R.B.var_block, (const u8 *)c->d_ref, (const u8 *)p->pool,
                       (int)c->k, haploid, view(c, MG_BF_ALT), view(c), (u32)c->map.rows_total, (u8 *)d_overflow_out, R.gen_list, c->d_gen_count, (unsigned short *)R.B.rec_class, tiles);
    HIP_TRY(c, hipGetLastError());
    c->map.rows_total += n;
    unsigned long long *d_cursor = c->d_gen_count + 1;
    // pass 1: how many exact-map insertion rows the other records need; which of them go to tier 3, which to the host
    HIP_TRY(c, hipMemsetAsync(R.round_counters, 0, 8 * FW_ROUND_COUNTERS * R.n_rounds, c->stream));
    TRY(blocks_tier2<1>(R, nullptr, (u8 *)d_overflow_out, d_cursor, 0u, nullptr));
    HIP_TRY(c, hipMemsetAsync(c->d_gen_count + 4, 0, 8, c->stream)); // (tier 3's count, before it compacts)
    TRY(blocks_tier3<1>(R, true, nullptr, (u8 *)d_overflow_out, d_cursor, 0u, nullptr));
    unsigned long long rows = 0;
    HIP_TRY(c, hipMemcpyAsync(&rows, d_cursor, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (rows) TRY(map_reserve(c, rows)); // between the passes
    // pass 2: insert.  Every REF k-mer takes the next insertion row of the batch (ids are then whatever order the
    // device reached them in: the index FILE, which every GPU of a call loads alike, is what fixes the counter layout).
    // The records keep the tier pass 1 gave them (its flags stand), so the rows counted are the rows used.
    HIP_TRY(c, hipMemsetAsync(d_cursor, 0, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(R.round_counters, 0, 8 * FW_ROUND_COUNTERS * R.n_rounds, c->stream));
    TRY(blocks_tier2<2>(R, nullptr, (u8 *)d_overflow_out, d_cursor, (u32)c->map.rows_total, nullptr));
    TRY(blocks_tier3<2>(R, false, nullptr, (u8 *)d_overflow_out, d_cursor, (u32)c->map.rows_total, nullptr));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->map.rows_total += rows;
    return MG_OK;
}

namespace {
int index_blocks_host(mg_ctx *c, const mg_blocks_host &x, int haploid, uint8_t *overflow_out)
{
    const DeviceGuard on_device(c);
    if (x.n_vars == 0) return MG_OK;
    if (!overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (c->bf[MG_BF_ALT].mode) return fail(c, MG_ERR_STATE, "mg_index_blocks after mg_bf_finalize");
    mg_panel_dev p{};
    void *d_bo, *d_vb, *d_nb;
    TRY(upload_blocks(c, x, &p, &d_bo, &d_vb, &d_nb));
    void *d_ovf;
    TRY(scratch(c, c->s_irr, x.n_vars, &d_ovf));
    HIP_TRY(c, hipMemsetAsync(d_ovf, 0, x.n_vars, c->stream));
    TRY(mg_index_blocks_device(c, &p, d_bo, d_vb, d_nb, haploid, d_ovf));
    HIP_TRY(c, hipMemcpy(overflow_out, d_ovf, x.n_vars, hipMemcpyDeviceToHost));
    return MG_OK;
}
} // namespace
MG_EXPORT int mg_index_blocks(mg_ctx *c, const mg_blocks_host *x, int haploid, uint8_t *overflow_out)
{
    if (!c || !x) return MG_ERR_ARG;
    if (c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    return index_blocks_host(c, *x, haploid, overflow_out);
}

// index time: blocks of one variant whose alleles are all shorter than k (nearly every block of a SNP panel), on the device
MG_EXPORT int mg_index_isolated(mg_ctx *c, size_t n_vars, const uint64_t *pos, const uint32_t *var_allele_off, const uint32_t *allele_off,
                                const char *allele_pool, size_t pool_len, const uint64_t *present_mask, const uint8_t *flags, uint8_t *overflow_out)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (!c) return MG_ERR_ARG;
    if (n_vars == 0) return MG_OK;
    if (!pos || !var_allele_off || !allele_off || !allele_pool || !present_mask || !flags || !overflow_out) return fail(c, MG_ERR_ARG, "NULL argument");
    if (!c->d_ref) return fail(c, MG_ERR_STATE, "mg_reference_upload first");
    if (c->bf[MG_BF_ALT].mode) return fail(c, MG_ERR_STATE, "mg_index_isolated after mg_bf_finalize");
    if (c->map.rows_total + n_vars >= 0xFFFFFFFFULL) return fail(c, MG_ERR_LIMIT, "exact map: more than 2^32-1 insertion rows");
    const size_t na = var_allele_off[n_vars];
    for (size_t v = 0; v < n_vars; ++v) // every window the kernel will read lies inside the uploaded reference (as mg_call_isolated checks)
        if (flags[v] & 1) {
            const u32 a0 = var_allele_off[v];
            const u64 rs = allele_off[a0 + 1] - allele_off[a0];
            if (pos[v] < c->k / 2 || pos[v] + rs + (c->k + 1) / 2 > c->ref_len)
                return fail(c, MG_ERR_ARG, "variant %zu flagged eligible but its flanks leave the uploaded reference", v);
        }
    if (allele_off[na] > pool_len) return fail(c, MG_ERR_ARG, "allele offsets exceed the pool");
    TRY(map_reserve(c, n_vars)); // may grow and re-hash the table: before the kernel, never under it
    void *d_pos, *d_vo, *d_ao, *d_pool, *d_pm, *d_fl, *d_ovf;
    TRY(upload(c, c->s_rows, pos, 8 * n_vars, &d_pos));
    TRY(upload(c, c->s_aux, var_allele_off, 4 * (n_vars + 1), &d_vo));
    TRY(upload(c, c->s_misc[0], allele_off, 4 * (na + 1), &d_ao));
    TRY(upload(c, c->s_misc[1], allele_pool, pool_len, &d_pool));
    TRY(upload(c, c->s_misc[3], present_mask, 8 * n_vars, &d_pm));
    TRY(upload(c, c->s_misc[4], flags, n_vars, &d_fl));
    TRY(scratch(c, c->s_irr, n_vars, &d_ovf));
    c->gate_dirty = true;
    hipLaunchKernelGGL(iso_index_kernel, dim3(nblocks(n_vars)), dim3(TPB), 0, c->stream, (const u8 *)c->d_ref, (u64)n_vars, (const u64 *)d_pos, (const u32 *)d_vo,
                       (const u32 *)d_ao, (const u8 *)d_pool, (const u64 *)d_pm, (const u8 *)d_fl, (int)c->k, view(c, MG_BF_ALT), view(c), (u32)c->map.rows_total,
                       (u8 *)d_ovf);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(overflow_out, d_ovf, n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->map.rows_total += n_vars;
    return MG_OK;
}

namespace {
int reference_alloc(mg_ctx *c, size_t len)
{
    for (void *q : {(void *)c->d_ref, (void *)c->d_ref2, (void *)c->d_refbad})
        if (q) hipFree(q);
    c->d_ref = nullptr;
    c->d_ref2 = nullptr;
    c->d_refbad = nullptr;
    c->ref_len = 0;
    const size_t padded = (len + 63) / 64 * 64 + 256; // the pack kernel reads whole 32-byte groups, pack_span whole dwords around a window
    const u64 n_words = (len + 31) / 32 + 4;
    HIP_TRY(c, hipMalloc(&c->d_ref, padded));
    HIP_TRY(c, hipMalloc(&c->d_ref2, n_words * 8));
    HIP_TRY(c, hipMalloc(&c->d_refbad, n_words * 4));
    HIP_TRY(c, hipMemsetAsync(c->d_ref, 0, padded, c->stream));
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_reference_upload(mg_ctx *c, const char *ascii, size_t len)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || (len && !ascii)) return MG_ERR_ARG;
    TRY(reference_alloc(c, len));
    if (len) HIP_TRY(c, hipMemcpyAsync(c->d_ref, ascii, len, hipMemcpyHostToDevice, c->stream));
    TRY(reference_pack(c, c->d_ref, len, c->d_ref2, c->d_refbad));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ref_len = len;
    return MG_OK;
}
// the same from a buffer already on the device (a copy is kept: the caller's buffer may go)
MG_EXPORT int mg_reference_upload_device(mg_ctx *c, const void *d_ascii, size_t len)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c || (len && !d_ascii)) return MG_ERR_ARG;
    TRY(reference_alloc(c, len));
    if (len) HIP_TRY(c, hipMemcpyAsync(c->d_ref, d_ascii, len, hipMemcpyDeviceToDevice, c->stream));
    TRY(reference_pack(c, c->d_ref, len, c->d_ref2, c->d_refbad));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->ref_len = len;
    return MG_OK;
}

MG_EXPORT int mg_call_isolated_device(mg_ctx *c, size_t n_vars, const void *d_pos, const void *d_var_allele_off,
                                      const void *d_allele_off, const void *d_allele_pool, const void *d_freq,
                                      const void *d_present_mask, const void *d_flags, float error_rate, int max_cov, int haploid,
                                      void *d_cov_out, void *d_gt1, void *d_gt2, void *d_gq, void *d_status, void *d_probs,
                                      const void *d_var_gt_off)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_vars == 0) return MG_OK;
    if (!c->d_ref) return fail(c, MG_ERR_STATE, "mg_reference_upload first");
    if (!c->bf[0].mode) return fail(c, MG_ERR_STATE, "`bf` not finalised");
    if (!c->map.slots) TRY(map_reserve(c, 0));
    GenoParams p;
    TRY(fill_geno_params(c, error_rate, max_cov, haploid, &p));
    u32 *need_slow = (u32 *)(c->d_hit_count + 3); // a spare word of the scan's counter block, compared with a call number
    if (++c->iso_call_no == 0) c->iso_call_no = 1;  // (never 0: the scan clears the block) so that nothing has to reset it
    hipLaunchKernelGGL(iso_cover_kernel<false>, dim3(nblocks(2 * (u64)n_vars)), dim3(TPB), 0, c->stream, (const u8 *)c->d_ref, (const u64 *)c->d_ref2, (const u32 *)c->d_refbad, (u64)n_vars,
                       (const u64 *)d_pos, (const u32 *)d_var_allele_off, (const u32 *)d_allele_off, (const u8 *)d_allele_pool,
                       (const u64 *)d_present_mask, (const u8 *)d_flags, (int)c->k, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, need_slow,
                       c->iso_call_no);
    hipLaunchKernelGGL(iso_cover_kernel<true>, dim3(nblocks(2 * (u64)n_vars)), dim3(TPB), 0, c->stream, (const u8 *)c->d_ref, (const u64 *)c->d_ref2, (const u32 *)c->d_refbad, (u64)n_vars,
                       (const u64 *)d_pos, (const u32 *)d_var_allele_off, (const u32 *)d_allele_off, (const u8 *)d_allele_pool,
                       (const u64 *)d_present_mask, (const u8 *)d_flags, (int)c->k, view(c, MG_BF_ALT), view(c), (u32 *)d_cov_out, need_slow,
                       c->iso_call_no);
    hipLaunchKernelGGL(iso_genotype_kernel, dim3(nblocks(n_vars)), dim3(TPB), 0, c->stream, (u64)n_vars, (const u32 *)d_var_allele_off,
                       (const float *)d_freq, p, (const u32 *)d_cov_out, (i32 *)d_gt1, (i32 *)d_gt2, (i32 *)d_gq, (u8 *)d_status,
                       (double *)d_probs, (const u64 *)d_var_gt_off);
    HIP_TRY(c, hipGetLastError());
    return MG_OK;
}

MG_EXPORT int mg_call_isolated(mg_ctx *c, size_t n_vars, const uint64_t *pos, const uint32_t *var_allele_off,
                               const uint32_t *allele_off, const char *allele_pool, size_t pool_len, const float *freq,
                               const uint64_t *present_mask, const uint8_t *flags, float error_rate, int max_cov, int haploid,
                               uint32_t *cov_out, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status, double *probs,
                               const uint64_t *var_gt_off)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (n_vars == 0) return MG_OK;
    if (!pos || !var_allele_off || !allele_off || !allele_pool || !freq || !present_mask || !flags || !cov_out || !gt1 || !gt2 ||
        !gq || !status)
        return fail(c, MG_ERR_ARG, "NULL argument");
    if (probs && !var_gt_off) return fail(c, MG_ERR_ARG, "probs needs var_gt_off");
    const size_t na = var_allele_off[n_vars];
    // host-side contract checks: every window the kernel will read lies inside the uploaded reference
    for (size_t v = 0; v < n_vars; ++v)
        if (flags[v] & 1) {
            const u32 a0 = var_allele_off[v];
            const u64 rs = allele_off[a0 + 1] - allele_off[a0];
            // what iso_cover_kernel reads: k/2 bases before the site, ceil(k/2) after the REF allele (the buffer's
            // 64-byte padding absorbs the aligned dwords around them)
            if (pos[v] < c->k / 2 || pos[v] + rs + (c->k + 1) / 2 > c->ref_len)
                return fail(c, MG_ERR_ARG, "variant %zu flagged eligible but its flanks leave the uploaded reference", v);
        }
    if (allele_off[na] > pool_len) return fail(c, MG_ERR_ARG, "allele offsets exceed the pool");
    void *d_pos, *d_vo, *d_ao, *d_pool, *d_fr, *d_pm, *d_fl, *d_cov, *d_g1, *d_g2, *d_gq, *d_st;
    TRY(upload(c, c->s_rows, pos, 8 * n_vars, &d_pos));
    TRY(upload(c, c->s_aux, var_allele_off, 4 * (n_vars + 1), &d_vo));
    TRY(upload(c, c->s_misc[0], allele_off, 4 * (na + 1), &d_ao));
    TRY(upload(c, c->s_misc[1], allele_pool, pool_len, &d_pool));
    TRY(upload(c, c->s_misc[2], freq, 4 * na, &d_fr));
    TRY(upload(c, c->s_misc[3], present_mask, 8 * n_vars, &d_pm));
    TRY(upload(c, c->s_misc[4], flags, n_vars, &d_fl));
    TRY(scratch(c, c->s_out, 4 * na, &d_cov));
    TRY(scratch(c, c->s_misc[5], 4 * n_vars, &d_g1));
    TRY(scratch(c, c->s_misc[6], 4 * n_vars, &d_g2));
    TRY(scratch(c, c->s_misc[7], 4 * n_vars, &d_gq));
    TRY(scratch(c, c->s_irr, n_vars, &d_st));
    // raw likelihoods are staged in a device workspace either way (one exp() per genotype instead of two)
    std::vector<u64> goff_tmp;
    if (!var_gt_off) {
        goff_tmp.resize(n_vars + 1);
        goff_tmp[0] = 0;
        for (size_t v = 0; v < n_vars; ++v) {
            const u64 A = var_allele_off[v + 1] - var_allele_off[v];
            goff_tmp[v + 1] = goff_tmp[v] + (haploid ? A : A * (A + 1) / 2);
        }
        var_gt_off = goff_tmp.data();
    }
    const size_t ng = var_gt_off[n_vars];
    void *d_pr, *d_go;
    TRY(scratch(c, c->s_open[0], 8 * (ng ? ng : 1), &d_pr));
    TRY(upload(c, c->s_open[1], var_gt_off, 8 * (n_vars + 1), &d_go));
    TRY(mg_call_isolated_device(c, n_vars, d_pos, d_vo, d_ao, d_pool, d_fr, d_pm, d_fl, error_rate, max_cov, haploid, d_cov, d_g1,
                                d_g2, d_gq, d_st, d_pr, d_go));
    if (probs && ng) HIP_TRY(c, hipMemcpyAsync(probs, d_pr, 8 * ng, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cov_out, d_cov, 4 * na, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gt1, d_g1, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gt2, d_g2, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(gq, d_gq, 4 * n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(status, d_st, n_vars, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

// ---- index payloads ---------------------------------------------------------------------------

// ---- panel genotypes from VCF text (gt_text_kernels.h) ------------------------------------------------------------------
MG_EXPORT int mg_decode_gt_text(mg_ctx *c, const char *text, size_t text_bytes, size_t n_records, const uint64_t *span_off, const uint32_t *span_len,
                                const int32_t *gt_index, uint32_t n_columns, const uint8_t *keep, int haploid, uint16_t *sp_default, uint32_t *sp_off,
                                uint64_t *raw_mask, uint32_t *max_allele, uint64_t *n_entries)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    c->gt_records = 0;
    c->gt_entries = 0;
    if (!sp_default || !sp_off || !n_entries) return fail(c, MG_ERR_ARG, "NULL argument");
    *n_entries = 0;
    *sp_default = (uint16_t)(1u << 14);
    sp_off[0] = 0;
    if (n_records == 0) return MG_OK;
    if (!span_off || !span_len || !gt_index || !raw_mask || !max_allele || (text_bytes && !text)) return fail(c, MG_ERR_ARG, "NULL argument");
    if (n_columns == 0) return fail(c, MG_ERR_ARG, "mg_decode_gt_text: no sample columns");
    std::vector<u32> rank(n_columns, 0xFFFFFFFFu);
    u32 n_keep = 0;
    for (u32 i = 0; i < n_columns; ++i)
        if (!keep || keep[i]) rank[i] = n_keep++;
    if (n_keep == 0) return fail(c, MG_ERR_ARG, "mg_decode_gt_text: no sample kept");
    if (n_records >= 0xFFFFFFFFull || (u64)n_records * n_keep > (1ull << 31)) return fail(c, MG_ERR_LIMIT, "mg_decode_gt_text takes at most 2^31 genotypes per batch");
    // the part of the text the spans lie in
    u64 lo = ~0ull, hi = 0;
    for (size_t r = 0; r < n_records; ++r) {
        if (span_off[r] > text_bytes || span_len[r] > text_bytes - span_off[r]) return fail(c, MG_ERR_ARG, "record %zu: sample columns outside the text", r);
        if (gt_index[r] < 0 || gt_index[r] > 1000) return fail(c, MG_ERR_ARG, "record %zu: GT index %d", r, gt_index[r]);
        if (!span_len[r]) continue;
        lo = std::min<u64>(lo, span_off[r]);
        hi = std::max<u64>(hi, span_off[r] + span_len[r]);
    }
    if (lo > hi) lo = hi = 0;
    std::vector<unsigned long long> off(n_records);
    for (size_t r = 0; r < n_records; ++r) off[r] = span_len[r] ? span_off[r] - lo : 0;
    void *d_text, *d_off, *d_len, *d_gi, *d_rank, *d_tok, *d_words, *d_stats;
    { // the text goes through a pinned staging buffer: one memcpy at memory speed, then one DMA
        const size_t nb = hi - lo;
        if (nb > c->h_gt_stage_cap) {
            if (c->h_gt_stage) hipHostFree(c->h_gt_stage);
            c->h_gt_stage = nullptr;
            c->h_gt_stage_cap = 0;
            HIP_TRY(c, hipHostMalloc(&c->h_gt_stage, nb + nb / 4 + 4096, hipHostMallocDefault));
            c->h_gt_stage_cap = nb + nb / 4 + 4096;
        }
        if (nb) memcpy(c->h_gt_stage, text + lo, nb);
        TRY(upload(c, c->s_gt[0], c->h_gt_stage, nb, &d_text));
    }
    TRY(upload(c, c->s_gt[1], off.data(), 8 * n_records, &d_off));
    TRY(upload(c, c->s_gt[2], span_len, 4 * n_records, &d_len));
    TRY(upload(c, c->s_gt[3], gt_index, 4 * n_records, &d_gi));
    TRY(upload(c, c->s_gt[4], rank.data(), 4 * (size_t)n_columns, &d_rank));
    const unsigned grid = (unsigned)std::min<u64>(n_records, 1024);
    TRY(scratch(c, c->s_gt[5], 8 * (size_t)grid * n_keep, &d_tok));
    TRY(scratch(c, c->s_gt[6], 2 * (size_t)n_records * n_keep, &d_words));
    TRY(scratch(c, c->s_gt[7], sizeof(GtStats) * n_records, &d_stats));
    hipLaunchKernelGGL(gt_decode_kernel, dim3(grid), dim3(GT_TPB), 0, c->stream, (const char *)d_text, (const unsigned long long *)d_off, (const u32 *)d_len,
                       (const i32 *)d_gi, (u32)n_records, n_columns, (const u32 *)d_rank, n_keep, haploid, (unsigned long long *)d_tok, (uint16_t *)d_words,
                       (GtStats *)d_stats);
    HIP_TRY(c, hipGetLastError());
    std::vector<GtStats> st(n_records);
    HIP_TRY(c, hipMemcpyAsync(st.data(), d_stats, sizeof(GtStats) * n_records, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (also: the host vectors uploaded above may go)
    // the default word: 0|0 phased or 0/0, whichever the batch holds more of
    u64 p0 = 0, u0 = 0;
    for (const GtStats &g : st) {
        p0 += g.n_phased0;
        u0 += g.n_unphased0;
    }
    const u32 dflt = u0 > p0 ? 0u : 1u << 14;
    u64 total = 0;
    for (size_t r = 0; r < n_records; ++r) {
        raw_mask[r] = st[r].raw_mask;
        max_allele[r] = st[r].max_allele;
        total += n_keep - (dflt ? st[r].n_phased0 : st[r].n_unphased0);
        if (total > 0xFFFFFFFFull) return fail(c, MG_ERR_LIMIT, "mg_decode_gt_text: 2^32 or more entries in one batch");
        sp_off[r + 1] = (u32)total;
    }
    *sp_default = (uint16_t)dflt;
    *n_entries = total;
    c->gt_records = (u32)n_records;
    c->gt_keep = n_keep;
    c->gt_default = dflt;
    c->gt_entries = total;
    void *d_spoff;
    TRY(upload(c, c->s_gt[8], sp_off, 4 * (n_records + 1), &d_spoff));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}
MG_EXPORT int mg_decode_gt_entries(mg_ctx *c, uint32_t *sp_sample, uint16_t *sp_gt)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if (!c->gt_records) return fail(c, MG_ERR_STATE, "mg_decode_gt_entries follows a mg_decode_gt_text that decoded something");
    if (!c->gt_entries) return MG_OK;
    if (!sp_sample || !sp_gt) return fail(c, MG_ERR_ARG, "NULL argument");
    void *d_s, *d_g;
    TRY(scratch(c, c->s_gt[5], 4 * c->gt_entries, &d_s)); // (the token scratch is free again)
    TRY(scratch(c, c->s_gt[9], 2 * c->gt_entries, &d_g));
    hipLaunchKernelGGL(gt_compact_kernel, dim3(std::min<u32>(c->gt_records, 2048)), dim3(GT_TPB), 0, c->stream, (const uint16_t *)c->s_gt[6].p, c->gt_records, c->gt_keep,
                       c->gt_default, (const u32 *)c->s_gt[8].p, (u32 *)d_s, (uint16_t *)d_g);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(sp_sample, d_s, 4 * c->gt_entries, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sp_gt, d_g, 2 * c->gt_entries, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_bf_export(mg_ctx *c, int which, uint64_t *words_out, uint16_t *counts_out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    BFState &b = c->bf[which];
    if (words_out) HIP_TRY(c, hipMemcpy(words_out, b.words, b.nwords * 8, hipMemcpyDeviceToHost));
    if (counts_out && b.mode && b.nset) {
        void *d16;
        TRY(scratch(c, c->s_out, b.nset * 2, &d16));
        const u32 *src = b.counts;
        if (which == MG_BF_ALT && c->coh_planes) { // the selected plane
            void *d32;
            TRY(scratch(c, c->s_aux, b.nset * 4, &d32));
            TRY(plane_gather(c, (u32 *)d32, nullptr));
            src = (const u32 *)d32;
        }
        hipLaunchKernelGGL(mask_u16_kernel, dim3(nblocks(b.nset)), dim3(TPB), 0, c->stream, src, (uint16_t *)d16,
                           b.nset);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(counts_out, d16, b.nset * 2, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return MG_OK;
}
MG_EXPORT int mg_bf_import(mg_ctx *c, int which, int mode, uint64_t size_bits, const uint64_t *words, const uint16_t *counts,
                           uint64_t n_counts)
{
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (c && (which == MG_BF_ALT || which == MG_BF_CTX)) c->bf[which].pos_set_valid = false;
    const DeviceGuard on_device(c);
    TRY(check_which(c, which));
    BFState &b = c->bf[which];
    if (size_bits != b.size) return fail(c, MG_ERR_ARG, "filter size %llu does not match the context (%llu)",
                                         (unsigned long long)size_bits, (unsigned long long)b.size);
    if (!words) return fail(c, MG_ERR_ARG, "words is NULL");
    HIP_TRY(c, hipMemcpy(b.words, words, b.nwords * 8, hipMemcpyHostToDevice));
    b.mode = 0;
    if (which == MG_BF_ALT) { // the gate follows the bits: rebuild it from them and from the map's keys
        TRY(alloc_gate(c));
        hipLaunchKernelGGL(gate_from_bits_kernel, dim3(nblocks(b.nwords)), dim3(TPB), 0, c->stream, view(c, MG_BF_ALT), b.nwords);
        if (c->map.slots)
            hipLaunchKernelGGL(map_gate_kernel, dim3(nblocks(1ULL << c->map.cap_log2)), dim3(TPB), 0, c->stream, view(c),
                               view(c, MG_BF_ALT));
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (mode) {
        TRY(mg_bf_finalize(c, which)); // rank is rebuilt on load, as bloom_filter.hpp:143 does
        if (n_counts != b.nset) return fail(c, MG_ERR_ARG, "counter count %llu != popcount %llu", (unsigned long long)n_counts,
                                            (unsigned long long)b.nset);
        if (n_counts) {
            void *d16;
            TRY(upload(c, c->s_out, counts, n_counts * 2, &d16));
            hipLaunchKernelGGL(widen_u16_kernel, dim3(nblocks(n_counts)), dim3(TPB), 0, c->stream, (const uint16_t *)d16, b.counts,
                               n_counts);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    return MG_OK;
}

// Sparse payloads: a filter is a few million set bits in 2^33..2^37, so the index file stores the
// ascending positions of the set bits (= counter order) instead of gigabytes of zeros.
MG_EXPORT int mg_bf_export_sparse(mg_ctx *c, int which, uint64_t *positions_out, uint16_t *counts_out)
{
    const DeviceGuard on_device(c, KEEP);
    TRY(check_which(c, which));
    BFState &b = c->bf[which];
    if (!b.mode) return fail(c, MG_ERR_STATE, "sparse export needs the filter finalised (rank directory)");
    if (positions_out && b.nset) {
        void *d;
        TRY(scratch(c, c->s_open[0], b.nset * 8, &d));
        hipLaunchKernelGGL(bit_positions_kernel, dim3(nblocks(b.nwords)), dim3(TPB), 0, c->stream, view(c, which), b.nwords, (u64 *)d);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(positions_out, d, b.nset * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (counts_out) return mg_bf_export(c, which, nullptr, counts_out);
    return MG_OK;
}
MG_EXPORT int mg_bf_import_sparse(mg_ctx *c, int which, int mode, uint64_t size_bits, const uint64_t *positions,
                                  const uint16_t *counts, uint64_t n)
{
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    if (c && (which == MG_BF_ALT || which == MG_BF_CTX)) c->bf[which].pos_set_valid = false;
    const DeviceGuard on_device(c);
    TRY(check_which(c, which));
    BFState &b = c->bf[which];
    if (size_bits != b.size) return fail(c, MG_ERR_ARG, "filter size %llu does not match the context (%llu)",
                                         (unsigned long long)size_bits, (unsigned long long)b.size);
    if (n && !positions) return fail(c, MG_ERR_ARG, "positions is NULL");
    HIP_TRY(c, hipMemsetAsync(b.words, 0, b.nwords * 8, c->stream));
    b.mode = 0;
    if (which == MG_BF_ALT) {
        TRY(alloc_gate(c));
        if (c->map.slots)
            hipLaunchKernelGGL(map_gate_kernel, dim3(nblocks(1ULL << c->map.cap_log2)), dim3(TPB), 0, c->stream, view(c),
                               view(c, MG_BF_ALT));
        c->gate_dirty = true;
    }
    if (n) {
        void *d;
        int *d_bad = (int *)(c->d_hit_count + 3);
        TRY(upload(c, c->s_open[0], positions, n * 8, &d));
        HIP_TRY(c, hipMemsetAsync(d_bad, 0, 4, c->stream));
        hipLaunchKernelGGL(set_bits_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, view(c, which), (const u64 *)d, (u64)n, b.size,
                           d_bad);
        HIP_TRY(c, hipGetLastError());
        int bad = 0;
        HIP_TRY(c, hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (bad) return fail(c, MG_ERR_ARG, "bit positions must be strictly ascending and below the filter size");
    }
    if (mode) {
        TRY(mg_bf_finalize(c, which));
        if (b.nset != n) return fail(c, MG_ERR_ARG, "popcount %llu != positions %llu", (unsigned long long)b.nset, (unsigned long long)n);
        if (n && counts) {
            void *d16;
            TRY(upload(c, c->s_out, counts, n * 2, &d16));
            hipLaunchKernelGGL(widen_u16_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const uint16_t *)d16, b.counts, (u64)n);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    return MG_OK;
}

namespace {
void unpack_lform(u64 lo, u64 hi, u32 k, char *out)
{
    static const char L[4] = {'A', 'C', 'G', 'T'};
    for (u32 i = 0; i < k; ++i) out[i] = L[(i < 32 ? lo >> (2 * i) : hi >> (2 * (i - 32))) & 3];
    out[k] = 0;
}
} // namespace

// The table's keys first (all k long: pack_regular sends every row of another length, pure ACGT or not, to the host's
// list, because a shorter or longer key cannot be told apart once packed), then the host's list.  Rows are expected to be
// k long, as every signature k-mer of the reference is; a key of the list that is longer needs a wider row than k + 1.
MG_EXPORT int mg_map_export(mg_ctx *c, char *rows_out, size_t stride, int32_t *vals_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    std::vector<u64> lo, hi;
    std::vector<u32> ids;
    TRY(map_dump(c, &lo, &hi, &ids));
    if (!rows_out && !vals_out) return MG_OK;
    if (stride < c->k + 1) return fail(c, MG_ERR_ARG, "stride %zu < k+1", stride);
    if (rows_out)
        for (auto &kv : c->map.irregular) // (a key other than k long: a row that cut it short would name another key)
            if (kv.first.size() + 1 > stride) return fail(c, MG_ERR_ARG, "stride %zu < a key of %zu bytes + NUL", stride, kv.first.size());
    std::vector<u32> vals(c->map.rows_total);
    if (c->map.rows_total && c->coh_planes) { // the selected plane
        void *d32;
        TRY(scratch(c, c->s_aux, c->map.rows_total * 4, &d32));
        TRY(plane_gather(c, nullptr, (u32 *)d32));
        HIP_TRY(c, hipMemcpyAsync(vals.data(), d32, c->map.rows_total * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    } else if (c->map.rows_total) HIP_TRY(c, hipMemcpy(vals.data(), c->map.vals, c->map.rows_total * 4, hipMemcpyDeviceToHost));
    size_t j = 0;
    for (; j < lo.size(); ++j) {
        if (rows_out) {
            memset(rows_out + j * stride, 0, stride);
            unpack_lform(lo[j], hi[j], c->k, rows_out + j * stride);
        }
        if (vals_out) vals_out[j] = (int32_t)vals[ids[j]];
    }
    for (auto &kv : c->map.irregular) {
        if (rows_out) {
            memset(rows_out + j * stride, 0, stride);
            memcpy(rows_out + j * stride, kv.first.data(), kv.first.size() < stride - 1 ? kv.first.size() : stride - 1);
        }
        if (vals_out) vals_out[j] = kv.second;
        ++j;
    }
    return MG_OK;
}
MG_EXPORT int mg_map_import(mg_ctx *c, const char *rows, size_t stride, size_t n, const int32_t *vals)
{
    const DeviceGuard on_device(c);
    if (c && c->coh_planes) return fail(c, MG_ERR_STATE, "%s: not while the context is in cohort mode (mg_cohort_end first)", __func__);
    TRY(check_rows(c, rows, stride, n));
    if (n == 0) return MG_OK;
    TRY(mg_map_insert(c, rows, stride, n));
    if (vals) {
        // values go through a lookup of each key (a file may repeat a key, or name one that was already present:
        // the counter of a key is the one its first insertion row owns, and the last row that names the key gives
        // its value); irregular rows live in the host list under the canonical form KMAP::canonical gives them
        // (kmap.hpp:86-97), and the loop below takes them in row order
        std::vector<u8> irr(n);
        void *d_rows, *d_vals, *d_last, *d_irr;
        const u64 n_ids = c->map.rows_total; // (>= n: the insert above has counted these rows)
        TRY(upload(c, c->s_rows, rows, stride * n, &d_rows));
        TRY(upload(c, c->s_aux, vals, 4 * n, &d_vals));
        TRY(scratch(c, c->s_misc[7], 4 * n_ids, &d_last));
        TRY(scratch(c, c->s_irr, n, &d_irr));
        HIP_TRY(c, hipMemsetAsync(d_last, 0, 4 * n_ids, c->stream));
        hipLaunchKernelGGL(map_set_kernel<0>, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const u8 *)d_rows, stride, n, view(c), view(c, MG_BF_ALT),
                           (const u32 *)d_vals, (u32 *)d_last, (u8 *)d_irr);
        hipLaunchKernelGGL(map_set_kernel<1>, dim3(nblocks(n)), dim3(TPB), 0, c->stream, (const u8 *)d_rows, stride, n, view(c), view(c, MG_BF_ALT),
                           (const u32 *)d_vals, (u32 *)d_last, (u8 *)d_irr);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(irr.data(), d_irr, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n; ++i)
            if (irr[i]) {
                auto it = c->map.irregular.find(host_irregular_key(rows + i * stride, stride));
                if (it != c->map.irregular.end()) it->second = vals[i];
            }
    }
    return MG_OK;
}

// ---- counting from reads: the KMC step of MALVA:104-110 fused into the call-time scan (main.cpp:482-500) ----------------------

namespace {
struct ReadsSeg { // one chunk, packed (pack_word): it stays on the device until the passes of mg_reads_finish have read it
    u64 n = 0;
    u64 *codes = nullptr;
    u32 *bad = nullptr;
};
struct ReadsTable { // the kept rows of one pass (what the scan took; mg_reads_export)
    u64 *hi = nullptr, *lo = nullptr;
    u32 *cnt = nullptr;
    u64 n = 0;
};
struct ReadsTiming {
    int phase; // 0 pack, 1 window + filter (counting pre-pass), 2 file, 3 reduce, 4 scan
    hipEvent_t a, b;
};
} // namespace
struct ReadsState {
    u32 min_count = 2, max_count = 255, part = 0, n_parts = 1, n_bins = RD_PARTS;
    bool finished = false;
    std::vector<ReadsSeg> segs;
    u32 *d_parts = nullptr;               // [RD_PARTS] gate survivors per partition (reads_window_kernel<0>)
    unsigned long long *d_meta = nullptr; // [0] windows inside ACGT, [1] survivors, [2] kept rows of the current pass
    std::vector<ReadsTable> kept;
    std::vector<ReadsTiming> tm;
    u64 bases = 0, windows = 0, survivors = 0, n_kept = 0, passes = 0;
    float ms[5] = {0, 0, 0, 0, 0};
    int slot = 0;
    bool slot_used[2] = {false, false};
    Scratch ascii[2], pairs[3], bin_base, bin_fill, out[3];
};

namespace {
bool reads_unfinished(const mg_ctx *c) { return c->reads && !c->reads->finished; }
void reads_drop(mg_ctx *c)
{
    ReadsState *R = c->reads;
    if (!R) return;
    hipStreamSynchronize(c->stream);
    for (auto &s : R->segs) {
        hipFree(s.codes);
        hipFree(s.bad);
    }
    for (auto &t : R->kept) {
        hipFree(t.hi);
        hipFree(t.lo);
        hipFree(t.cnt);
    }
    for (auto &t : R->tm) {
        if (t.a) hipEventDestroy(t.a);
        if (t.b) hipEventDestroy(t.b);
    }
    hipFree(R->d_parts);
    hipFree(R->d_meta);
    for (Scratch *s : {&R->ascii[0], &R->ascii[1], &R->pairs[0], &R->pairs[1], &R->pairs[2], &R->bin_base, &R->bin_fill, &R->out[0], &R->out[1], &R->out[2]})
        hipFree(s->p);
    delete R;
    c->reads = nullptr;
}
int reads_open(mg_ctx *c)
{
    if (!c) return MG_ERR_ARG;
    if (!c->reads) return fail(c, MG_ERR_STATE, "mg_reads_begin first");
    if (c->reads->finished) return fail(c, MG_ERR_STATE, "mg_reads_finish has run: mg_reads_begin starts a new count");
    return MG_OK;
}
int reads_event(mg_ctx *c, hipEvent_t *e)
{
    HIP_TRY(c, hipEventCreate(e));
    HIP_TRY(c, hipEventRecord(*e, c->stream));
    return MG_OK;
}
template <int MODE>
void launch_reads_windows(mg_ctx *c, const ReadsSeg &s, const ReadsPass &rp)
{
    if (s.n < c->ref_k) return;
    const u64 nw = s.n - c->ref_k + 1;
    const unsigned grid = (unsigned)std::min<u64>(nblocks((nw + RD_W - 1) / RD_W), 1u << 16);
    const BFView bf = view(c, MG_BF_ALT);
    if (c->k == 35 && c->ref_k == 43)
        hipLaunchKernelGGL((reads_window_kernel<35, 43, MODE>), dim3(grid), dim3(TPB), 0, c->stream, s.codes, s.bad, nw, (int)c->k, (int)c->ref_k, bf, rp);
    else if (c->k == 35 && c->ref_k == 63)
        hipLaunchKernelGGL((reads_window_kernel<35, 63, MODE>), dim3(grid), dim3(TPB), 0, c->stream, s.codes, s.bad, nw, (int)c->k, (int)c->ref_k, bf, rp);
    else
        hipLaunchKernelGGL((reads_window_kernel<0, 0, MODE>), dim3(grid), dim3(TPB), 0, c->stream, s.codes, s.bad, nw, (int)c->k, (int)c->ref_k, bf, rp);
}
// a chunk already on the device (4-byte aligned): packed into a segment of its own, its survivors counted per partition
int reads_add_dev(mg_ctx *c, const u8 *d_ascii, size_t bytes)
{
    ReadsState &R = *c->reads;
    const u64 n_words = (bytes + 31) / 32 + 4; // (+ the words the window loads may touch past the last base)
    R.segs.push_back(ReadsSeg{});
    ReadsSeg &s = R.segs.back();
    s.n = bytes;
    HIP_TRY(c, hipMalloc(&s.codes, n_words * 8));
    HIP_TRY(c, hipMalloc(&s.bad, n_words * 4));
    ReadsTiming t0{0, nullptr, nullptr}, t1{1, nullptr, nullptr};
    TRY(reads_event(c, &t0.a));
    hipLaunchKernelGGL(reads_pack_kernel, dim3(nblocks(n_words)), dim3(TPB), 0, c->stream, d_ascii, (u64)bytes, s.codes, s.bad, n_words);
    TRY(reads_event(c, &t0.b));
    ReadsPass rp{};
    rp.part = R.part;
    rp.n_parts = R.n_parts;
    rp.bin_mask = R.n_bins - 1;
    rp.part_count = R.d_parts;
    rp.meta = R.d_meta;
    launch_reads_windows<0>(c, s, rp);
    HIP_TRY(c, hipGetLastError());
    TRY(reads_event(c, &t1.b));
    R.tm.push_back(t0);
    R.tm.push_back(t1); // (no `a`: it starts where the pack ended)
    R.bases += bytes;
    return MG_OK;
}
int reads_timings(mg_ctx *c)
{
    ReadsState &R = *c->reads;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipEvent_t prev = nullptr;
    for (auto &t : R.tm) {
        float ms = 0;
        HIP_TRY(c, hipEventElapsedTime(&ms, t.a ? t.a : prev, t.b));
        R.ms[t.phase] += ms;
        prev = t.b;
    }
    return MG_OK;
}
} // namespace

MG_EXPORT int mg_reads_begin(mg_ctx *c, uint32_t min_count, uint32_t max_count, uint32_t part, uint32_t n_parts)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (c->ref_k > MG_MAX_PACKED_K) return fail(c, MG_ERR_LIMIT, "counting reads supports ref_k <= %d (ref_k = %u), as the KMC database path does", MG_MAX_PACKED_K, c->ref_k);
    if (n_parts == 0 || part >= n_parts) return fail(c, MG_ERR_ARG, "key partition %u of %u", part, n_parts);
    if (!c->bf[0].mode || !c->bf[1].mode) return fail(c, MG_ERR_STATE, "mg_reads_begin needs both filters finalised (the scan's gate decides what is counted)");
    reads_drop(c);
    c->reads = new ReadsState();
    ReadsState &R = *c->reads;
    R.min_count = min_count ? min_count : 1; // (KMC: -ci0 keeps what -ci1 keeps)
    R.max_count = max_count ? max_count : 1;
    R.part = part;
    R.n_parts = n_parts;
    R.n_bins = 1u << c->reads_parts_log2;
    HIP_TRY(c, hipMalloc(&R.d_parts, (size_t)RD_PARTS * 4));
    HIP_TRY(c, hipMalloc(&R.d_meta, 32));
    HIP_TRY(c, hipMemsetAsync(R.d_parts, 0, (size_t)RD_PARTS * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(R.d_meta, 0, 32, c->stream));
    TRY(pipeline_ready(c));
    return MG_OK;
}

// Whole records, any byte outside ACGT (a newline) between two of them.  The bytes go up on the copy stream into one of two
// slots (a pinned source -- mg_host_alloc -- makes that a DMA beside the device's work); the call returns once they are
// up, while the pack and the pre-pass of this chunk run behind on the context's stream.
MG_EXPORT int mg_reads_add(mg_ctx *c, const char *seq, size_t bytes)
{
    const DeviceGuard on_device(c, LAZY);
    TRY(reads_open(c));
    if (bytes == 0) return MG_OK;
    if (!seq) return fail(c, MG_ERR_ARG, "NULL reads");
    ReadsState &R = *c->reads;
    const int sl = R.slot;
    R.slot ^= 1;
    const size_t want = (bytes + 63) / 64 * 64 + 256;
    if (want > R.ascii[sl].cap) HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the slot is about to be freed and reallocated)
    void *d;
    TRY(scratch(c, R.ascii[sl], want, &d));
    if (R.slot_used[sl]) HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->ev_free[sl], 0)); // the pack that read this slot is done
    HIP_TRY(c, hipMemcpyAsync(d, seq, bytes, hipMemcpyHostToDevice, c->copy_stream));
    HIP_TRY(c, hipEventRecord(c->ev_up[sl], c->copy_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_up[sl], 0));
    TRY(reads_add_dev(c, (const u8 *)d, bytes));
    HIP_TRY(c, hipEventRecord(c->ev_free[sl], c->stream));
    R.slot_used[sl] = true;
    HIP_TRY(c, hipEventSynchronize(c->ev_up[sl])); // the caller may reuse its buffer
    return MG_OK;
}

MG_EXPORT int mg_reads_add_device(mg_ctx *c, const void *d_seq, size_t bytes)
{
    const DeviceGuard on_device(c, LAZY);
    TRY(reads_open(c));
    if (bytes == 0) return MG_OK;
    if (!d_seq) return fail(c, MG_ERR_ARG, "NULL reads");
    if (((uintptr_t)d_seq & 3) == 0) return reads_add_dev(c, (const u8 *)d_seq, bytes);
    ReadsState &R = *c->reads; // (the pack reads whole dwords: an unaligned source is copied first)
    const int sl = R.slot;
    R.slot ^= 1;
    const size_t want = (bytes + 63) / 64 * 64 + 256;
    if (want > R.ascii[sl].cap) HIP_TRY(c, hipStreamSynchronize(c->stream));
    void *d;
    TRY(scratch(c, R.ascii[sl], want, &d));
    HIP_TRY(c, hipMemcpyAsync(d, d_seq, bytes, hipMemcpyDeviceToDevice, c->stream));
    TRY(reads_add_dev(c, (const u8 *)d, bytes));
    HIP_TRY(c, hipEventRecord(c->ev_free[sl], c->stream));
    R.slot_used[sl] = true;
    return MG_OK;
}

// The passes: partitions grouped so that the pairs of one pass fit reads_budget_mb (at least reads_passes of them); per pass
// every chunk's survivors of those partitions are filed into their bins, each bin is reduced to its distinct keys, [min, max]
// applied, and the kept rows scanned by mg_kmc_scan_device -- the scan itself, not a second one.
MG_EXPORT int mg_reads_finish(mg_ctx *c, uint64_t *n_kept_out)
{
    const DeviceGuard on_device(c, LAZY);
    TRY(reads_open(c));
    ReadsState &R = *c->reads;
    R.finished = true;
    std::vector<u32> parts(RD_PARTS);
    unsigned long long meta[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(parts.data(), R.d_parts, (size_t)RD_PARTS * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(meta, R.d_meta, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    R.windows = meta[0];
    R.survivors = meta[1];
    // passes: runs of partitions whose pairs fit the budget (a partition is never split: a bin larger than the budget takes a pass
    // of its own); reads_passes cuts the partitions into that many equal ranges first
    const u64 per_pass = std::max<u64>(1, ((u64)c->reads_budget_mb << 20) / 20);
    const u32 range = c->reads_passes > 0 ? (R.n_bins + (u32)c->reads_passes - 1) / (u32)c->reads_passes : R.n_bins;
    struct Pass {
        u32 lo, hi;
        u64 pairs;
    };
    std::vector<Pass> plan;
    u64 biggest = 0;
    for (u32 p = 0; p < R.n_bins;) {
        const u32 end = std::min<u32>(R.n_bins, (p / range + 1) * range);
        u64 sum = 0;
        u32 q = p;
        while (q < end && (q == p || sum + parts[q] <= per_pass)) sum += parts[q++];
        if (sum) plan.push_back(Pass{p, q, sum});
        biggest = std::max(biggest, sum);
        p = q;
    }
    void *ph, *pl, *pc, *pbase, *pfill, *oh, *ol, *oc;
    if (biggest) {
        TRY(scratch(c, R.pairs[0], biggest * 8, &ph));
        TRY(scratch(c, R.pairs[1], biggest * 8, &pl));
        TRY(scratch(c, R.pairs[2], biggest * 4, &pc));
        TRY(scratch(c, R.out[0], biggest * 8, &oh));
        TRY(scratch(c, R.out[1], biggest * 8, &ol));
        TRY(scratch(c, R.out[2], biggest * 4, &oc));
        TRY(scratch(c, R.bin_base, (size_t)RD_PARTS * 8, &pbase));
        TRY(scratch(c, R.bin_fill, (size_t)RD_PARTS * 4, &pfill));
    }
    std::vector<u64> base(RD_PARTS);
    for (const Pass &ps : plan) {
        const u32 nb = ps.hi - ps.lo;
        u64 at = 0;
        for (u32 b = 0; b < nb; ++b) {
            base[b] = at;
            at += parts[ps.lo + b];
        }
        HIP_TRY(c, hipMemcpyAsync(pbase, base.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(pfill, 0, (size_t)nb * 4, c->stream));
        HIP_TRY(c, hipMemsetAsync(R.d_meta + 2, 0, 8, c->stream));
        ReadsTiming tf{2, nullptr, nullptr}, tr{3, nullptr, nullptr}, ts{4, nullptr, nullptr}; // (each event destroyed once: entries without `a` start at the previous entry's end)
        TRY(reads_event(c, &tf.a));
        ReadsPass rp{};
        rp.part = R.part;
        rp.n_parts = R.n_parts;
        rp.bin_mask = R.n_bins - 1;
        rp.p_lo = ps.lo;
        rp.p_hi = ps.hi;
        rp.bin_base = (const u64 *)pbase;
        rp.bin_fill = (u32 *)pfill;
        rp.key_hi = (u64 *)ph;
        rp.key_lo = (u64 *)pl;
        for (const ReadsSeg &s : R.segs) launch_reads_windows<1>(c, s, rp);
        HIP_TRY(c, hipGetLastError());
        TRY(reads_event(c, &tf.b));
        ReadsReduce rr{(const u64 *)pbase, (const u32 *)pfill, (u64 *)ph, (u64 *)pl, (u32 *)pc, R.min_count, R.max_count, (u64 *)oh, (u64 *)ol, (u32 *)oc, R.d_meta + 2};
        hipLaunchKernelGGL(reads_reduce_kernel, dim3(nb), dim3(RD_TPB), 0, c->stream, rr);
        HIP_TRY(c, hipGetLastError());
        TRY(reads_event(c, &tr.b));
        unsigned long long kept = 0;
        HIP_TRY(c, hipMemcpyAsync(&kept, R.d_meta + 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream)); // (also: `base` may be rewritten for the next pass)
        ReadsTable t;
        t.n = kept;
        R.kept.push_back(t);
        ReadsTable &kt = R.kept.back();
        if (kept) {
            HIP_TRY(c, hipMalloc(&kt.hi, kept * 8));
            HIP_TRY(c, hipMalloc(&kt.lo, kept * 8));
            HIP_TRY(c, hipMalloc(&kt.cnt, kept * 4));
            HIP_TRY(c, hipMemcpyAsync(kt.hi, oh, kept * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(kt.lo, ol, kept * 8, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(kt.cnt, oc, kept * 4, hipMemcpyDeviceToDevice, c->stream));
            TRY(reads_event(c, &ts.a));
            TRY(mg_kmc_scan_device(c, kt.hi, kt.lo, kt.cnt, kept));
            TRY(reads_event(c, &ts.b));
        }
        R.tm.push_back(tf);
        R.tm.push_back(ReadsTiming{3, nullptr, tr.b}); // (from where the filing ended)
        if (kept) R.tm.push_back(ts);
        R.n_kept += kept;
        ++R.passes;
    }
    TRY(reads_timings(c));
    if (n_kept_out) *n_kept_out = R.n_kept;
    return MG_OK;
}

MG_EXPORT int mg_reads_export(mg_ctx *c, uint64_t *hi, uint64_t *lo, uint32_t *cnt, size_t cap, uint64_t *n_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->reads || !c->reads->finished) return fail(c, MG_ERR_STATE, "mg_reads_finish first");
    const ReadsState &R = *c->reads;
    if (n_out) *n_out = R.n_kept;
    size_t at = 0;
    for (const ReadsTable &t : R.kept) {
        if (at >= cap) break;
        const size_t m = std::min<size_t>(t.n, cap - at);
        if (!m) continue;
        if (!hi || !lo || !cnt) return fail(c, MG_ERR_ARG, "NULL output");
        HIP_TRY(c, hipMemcpyAsync(hi + at, t.hi, m * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(lo + at, t.lo, m * 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(cnt + at, t.cnt, m * 4, hipMemcpyDeviceToHost, c->stream));
        at += m;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}

MG_EXPORT int mg_reads_stats(mg_ctx *c, float *ms_out, uint64_t *counts_out)
{
    const DeviceGuard on_device(c, LAZY);
    if (!c) return MG_ERR_ARG;
    if (!c->reads || !c->reads->finished) return fail(c, MG_ERR_STATE, "mg_reads_finish first");
    const ReadsState &R = *c->reads;
    if (ms_out)
        for (int i = 0; i < 5; ++i) ms_out[i] = R.ms[i];
    if (counts_out) {
        counts_out[0] = R.bases;
        counts_out[1] = R.windows;
        counts_out[2] = R.survivors;
        counts_out[3] = R.passes;
        counts_out[4] = R.n_kept;
    }
    return MG_OK;
}

// ---- introspection of the stores (tests): kept last, so that no other kernel moves in the code object -----------------------

namespace {
// what the call-time lookups read of the directory inside the records, one thread per filter slot (mg_debug_bucket_count)
__global__ void __launch_bounds__(TPB) bucket_debug_kernel(MapView m, BFView bf, const u64 *idx, u64 n, long long *rank, u32 *count)
{
    const u64 i = (u64)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    rank[i] = bucket_rank(m, idx[i]);
    count[i] = bucket_count(m, bf, idx[i]);
}
} // namespace

// launch_tile_scan on the caller's values, with the buffers mg_bf_finalize gives it
MG_EXPORT int mg_debug_tile_scan(mg_ctx *c, uint32_t *x, uint64_t n, uint64_t *total)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if ((n && !x) || !total) return fail(c, MG_ERR_ARG, "x or total is NULL");
    void *d_tiles;
    TRY(upload(c, c->s_misc[1], x, n * 4, &d_tiles));
    unsigned long long *d_total = c->d_hit_count, t = 0;
    TRY(launch_tile_scan(c, (u32 *)d_tiles, n, d_total));
    if (n) HIP_TRY(c, hipMemcpyAsync(x, d_tiles, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&t, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *total = t;
    return MG_OK;
}
// fmt_scan on the caller's row lengths, as encode_rows runs it behind a length pass: the text encoder's scratch, the meta block zeroed
// and, with `flag`, meta[1] raised as a length kernel raises it for a row of 4 GB or more
MG_EXPORT int mg_debug_row_scan(mg_ctx *c, const uint32_t *len, uint64_t n, int flag, uint64_t *row_off_out, uint64_t *total)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    if ((n && !len) || !row_off_out || !total) return fail(c, MG_ERR_ARG, "len, row_off_out or total is NULL");
    if (n >= (1ull << 32)) return fail(c, MG_ERR_LIMIT, "mg_debug_row_scan: more than 2^32 - 1 rows in one call");
    *total = 0;
    row_off_out[0] = 0;
    if (n == 0) return MG_OK;
    void *d_len, *d_meta, *part, *d_off;
    TRY(upload(c, c->s_enc[TM_FMT][ES_LEN], len, 4 * n, &d_len));
    TRY(scratch(c, c->s_enc[TM_FMT][ES_META], 16, &d_meta));
    const u64 n_part = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    TRY(scratch(c, c->s_scan, 8 * n_part, &part));
    TRY(scratch(c, c->stage[ST_ROW_OFF], 8 * (n + 1), &d_off));
    const unsigned long long raised[2] = {0, flag ? 1ull : 0ull};
    unsigned long long t = 0;
    HIP_TRY(c, hipMemcpyAsync(d_meta, raised, 16, hipMemcpyHostToDevice, c->stream));
    fmt_scan(c, d_len, n, n_part, part, d_off, (unsigned long long *)d_meta);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(row_off_out, d_off, 8 * (n + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&t, d_meta, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *total = t;
    return MG_OK;
}
// bucket_rank / bucket_count of filter slots, through the views a lookup launched now would get
MG_EXPORT int mg_debug_bucket_count(mg_ctx *c, const uint64_t *idx, uint64_t n, int64_t *rank_out, uint32_t *count_out)
{
    const DeviceGuard on_device(c, KEEP);
    if (!c) return MG_ERR_ARG;
    const BFState &b = c->bf[MG_BF_ALT];
    if (!b.mode || !c->map.slots) return fail(c, MG_ERR_STATE, "mg_debug_bucket_count needs `bf` finalised (the directory is written then)");
    if (n == 0) return MG_OK;
    if (!idx || !rank_out || !count_out) return fail(c, MG_ERR_ARG, "NULL pointer");
    for (u64 i = 0; i < n; ++i)
        if (idx[i] >= b.size) return fail(c, MG_ERR_ARG, "slot %llu is outside the filter (%llu bits)", (unsigned long long)idx[i], (unsigned long long)b.size);
    void *d_idx, *d_rank, *d_count;
    TRY(upload(c, c->s_misc[5], idx, n * 8, &d_idx));
    TRY(scratch(c, c->s_misc[6], n * 8, &d_rank));
    TRY(scratch(c, c->s_out, n * 4, &d_count));
    hipLaunchKernelGGL(bucket_debug_kernel, dim3(nblocks(n)), dim3(TPB), 0, c->stream, view(c), view(c, MG_BF_ALT), (const u64 *)d_idx, (u64)n, (long long *)d_rank,
                       (u32 *)d_count);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(rank_out, d_rank, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(count_out, d_count, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MG_OK;
}
