/*
 * malva_hip.h -- C ABI of the MI355X-native malva-geno hot path.
 *
 * The reference (AlgoLab/malva v1.3.1) has no plugin/FFI seam: its hot path is
 * the header-only classes BF (bloom_filter.hpp:52-157), KMAP (kmap.hpp:46-132)
 * and VB (var_block.hpp:61-798), driven one k-mer / one block at a time from
 * main.cpp.  This header is that seam, cut at exactly the calls index_main and
 * call_main make, with every per-k-mer call turned into a batch call.  Each
 * entry point cites the reference interface it replaces; INTEGRATION.md shows
 * the thin BF/KMAP/VB wrappers a maintainer would put in front of it.
 *
 * Conventions
 *   - every function returns 0 (MG_OK) or a negative MG_ERR_*; the message for
 *     the last failure on a context is mg_last_error(ctx).  Nothing throws.
 *   - all device memory is owned by the opaque mg_ctx (one context = one GPU).
 *     Calls on one context must be serialised by the caller, exactly like the
 *     single-threaded reference; they may come from any host thread (each entry
 *     point makes the context's GPU current for the calling thread and puts the
 *     previous one back), and different contexts may be driven concurrently.
 *   - "rows" arguments are host buffers of n fixed-stride ASCII k-mers, each
 *     NUL-terminated inside its stride (the reference passes `const char*`
 *     and measures with strlen, bloom_filter.hpp:69); 1 <= strlen <= 128.
 *     They may be reused as soon as the call returns.
 *   - the *_device variants take device pointers valid on the context's GPU
 *     and are asynchronous on the context's stream (mg_set_stream); everything
 *     else synchronises before returning.
 *   - packed k-mer tables (the KMC stream) are SoA {hi[], lo[], cnt[]}: the
 *     ref_k-mer as a 2-bit string (A=0 C=1 G=2 T=3), MSB-first and right
 *     aligned in the 128-bit value hi:lo, so integer order == strcmp order.
 *   - there is no CPU fallback anywhere behind this interface: without a
 *     usable HIP device mg_create fails.
 */
#ifndef MALVA_HIP_H
#define MALVA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_ERR_ARG (-1)    /* bad argument */
#define MG_ERR_HIP (-2)    /* HIP runtime / launch failure */
#define MG_ERR_STATE (-3)  /* call not valid in the filter's current mode */
#define MG_ERR_NOMEM (-4)  /* allocation failed */
#define MG_ERR_LIMIT (-5)  /* size beyond what the implementation addresses */
#define MG_ERR_COMM (-6)   /* RCCL unavailable or a collective failed */

#define MG_BF_ALT 0 /* `bf`         main.cpp:300 -- ALT-allele signature k-mers        */
#define MG_BF_CTX 1 /* `context_bf` main.cpp:302 -- reference contexts (ref_k-mers)    */

#define MG_MAX_KMER 128 /* longest ASCII k-mer a row may hold                            */
#define MG_MAX_PACKED_K 64 /* longest k / ref_k of the packed (2-bit) paths              */

typedef struct mg_ctx mg_ctx;

/* ---- lifetime ----------------------------------------------------------- */

/* BF bf(opt::bf_size); KMAP ref_bf; BF context_bf(opt::bf_size)  (main.cpp:300-302)
 * plus VB vb(opt::k, opt::error_rate) (main.cpp:305,520).  bf_bits is the size
 * of EACH filter in bits (-b N => N * 2^33, argument_parser.hpp:119-123). */
int mg_create(mg_ctx **out, int device, uint32_t k, uint32_t ref_k, uint64_t bf_bits);
int mg_destroy(mg_ctx *ctx);
const char *mg_last_error(const mg_ctx *ctx);
/* Launch everything on `hip_stream` (a hipStream_t; NULL = the context's own
 * stream).  Lets a caller time the kernels with events on its own stream.
 * NULL never means HIP's default stream: a caller that works on the legacy
 * default stream (handle 0 in most bindings) passes MG_STREAM_DEFAULT. */
#define MG_STREAM_DEFAULT ((void *)1) /* == hipStreamLegacy */
int mg_set_stream(mg_ctx *ctx, void *hip_stream);
int mg_synchronize(mg_ctx *ctx);

/* ---- BF  (bloom_filter.hpp:52-157) -------------------------------------- */

/* void BF::add_key(const char*)                        bloom_filter.hpp:81   */
int mg_bf_insert(mg_ctx *ctx, int which, const char *rows, size_t stride, size_t n);
/* bool BF::test_key(const char*) const                 bloom_filter.hpp:87   */
int mg_bf_test(mg_ctx *ctx, int which, const char *rows, size_t stride, size_t n, uint8_t *out);
/* void BF::switch_mode()                               bloom_filter.hpp:93
 * builds the rank directory and one zeroed counter per set bit */
int mg_bf_finalize(mg_ctx *ctx, int which);
/* bool BF::increment(const char*, uint32)              bloom_filter.hpp:100
 * returns MG_ERR_STATE where the reference returns false (write mode) */
int mg_bf_increment(mg_ctx *ctx, int which, const char *rows, size_t stride, size_t n, const uint32_t *counters);
/* uint16_t BF::get_count(const char*) const            bloom_filter.hpp:115
 * (0 for every row while the filter is still in write mode) */
int mg_bf_get_count(mg_ctx *ctx, int which, const char *rows, size_t stride, size_t n, uint16_t *out);
/* _size, popcount (== _counts.size() once finalised), _mode */
int mg_bf_info(mg_ctx *ctx, int which, uint64_t *size_bits, uint64_t *n_set, int *mode);

/* ---- KMAP  (kmap.hpp:46-132) -------------------------------------------- */

/* void KMAP::add_key(const char*)                      kmap.hpp:108          */
int mg_map_insert(mg_ctx *ctx, const char *rows, size_t stride, size_t n);
/* bool KMAP::test_key(const char*)                     kmap.hpp:99           */
int mg_map_test(mg_ctx *ctx, const char *rows, size_t stride, size_t n, uint8_t *out);
/* void KMAP::increment(const char*, int)               kmap.hpp:114          */
int mg_map_increment(mg_ctx *ctx, const char *rows, size_t stride, size_t n, const int32_t *counters);
/* int KMAP::get_count(const char*)                     kmap.hpp:124          */
int mg_map_get_count(mg_ctx *ctx, const char *rows, size_t stride, size_t n, int32_t *out);
/* kmers.size() */
int mg_map_size(mg_ctx *ctx, uint64_t *n_keys);

/* ---- index-time reference scan  (main.cpp:383-401) ----------------------- */

/* One used contig, upper-cased ASCII: for every position, if the centre k-mer
 * of the ref_k window hits `bf`, add the window to `context_bf`. */
int mg_ref_scan(mg_ctx *ctx, const char *contig, size_t len);
/* the same for a contig that already lies at [offset, offset + len) of the buffer given to mg_reference_upload (the
 * reference's index_main holds every contig in memory too, main.cpp:283-295): nothing crosses PCIe, asynchronous */
int mg_ref_scan_resident(mg_ctx *ctx, uint64_t offset, size_t len);

/* ---- call-time KMC scan  (main.cpp:482-500) ------------------------------ */

/* for each (ref_k-mer, count): ref_bf.increment(centre, count);
 * if (!context_bf.test_key(ref_k-mer)) bf.increment(centre, count).
 * Both filters must be finalised.  ref_k <= MG_MAX_PACKED_K. */
int mg_kmc_scan(mg_ctx *ctx, const uint64_t *hi, const uint64_t *lo, const uint32_t *cnt, size_t n);
int mg_kmc_scan_device(mg_ctx *ctx, const void *d_hi, const void *d_lo, const void *d_cnt, size_t n);

/* The same scan over COMPACT rows: 12 bytes per row instead of 20 -- three little-endian dwords holding the 96-bit
 * value  count << (2 ref_k) | ref_k-mer (2-bit string as above).  For 33 <= ref_k <= 44 (the reference's default is 43)
 * and counts below 2^(96 - 2 ref_k) (1024 at ref_k 43; KMC caps counts at 255, MALVA:107).  mg_kmc_pack_rows_device
 * builds them from an SoA table (n rounded up to a multiple of four rows: mg_kmc_rows_bytes(n) bytes, zero padded)
 * and returns MG_ERR_LIMIT when a count does not fit; the scan is asynchronous like mg_kmc_scan_device. */
size_t mg_kmc_rows_bytes(size_t n);
int mg_kmc_pack_rows_device(mg_ctx *ctx, const void *d_hi, const void *d_lo, const void *d_cnt, size_t n, void *d_rows_out);
int mg_kmc_scan_rows_device(mg_ctx *ctx, const void *d_rows, size_t n);

/* KMC database feed: CKMCFile::OpenForListing / ReadNextKmer / CKmerAPI::to_string (main.cpp:444-449, 482-490; the KMC
 * API is a third-party library the reference links, absent from its checkout: format restated from KMC's published
 * database layout, "parity unpinned" -- DESIGN.md).  The host hands over what the two files hold and parses nothing:
 *   mg_kmc_set_lut       <db>.kmc_pre: the prefix table (every bin's 4^lut_prefix_len entries, concatenated: first
 *                        record index of each prefix), record geometry and the [min_count, max_count] listing filter
 *   mg_kmc_scan_records  a run of raw <db>.kmc_suf records (suffix bytes + little-endian counter), `first_record` =
 *                        index of the first one in the database; decoded to table rows ON THE DEVICE (prefix from the
 *                        table, suffix from the record), then scanned as mg_kmc_scan does.  10 bytes per 43-mer cross
 *                        PCIe instead of 20.  Upload and scan of consecutive pieces overlap (two staging slots);
 *                        buffers from mg_host_alloc (pinned) make the uploads asynchronous.
 *   mg_kmc_decode_records  the decoded rows themselves (tests / inspection). */
int mg_host_alloc(void **out, size_t bytes);
int mg_host_free(void *p);
int mg_kmc_set_lut(mg_ctx *ctx, const uint64_t *lut, size_t n_lut, uint32_t lut_prefix_len, uint32_t suffix_bytes,
                   uint32_t counter_bytes, uint32_t min_count, uint64_t max_count, uint64_t total_records);
int mg_kmc_scan_records(mg_ctx *ctx, const void *records, size_t n, uint64_t first_record);
int mg_kmc_decode_records(mg_ctx *ctx, const void *records, size_t n, uint64_t first_record, uint64_t *hi_out,
                          uint64_t *lo_out, uint32_t *cnt_out);

/* ---- counting from reads: the KMC step of MALVA:104-110 fused into the call-time scan (main.cpp:482-500) ----------------
 * `kmc -k<ref_k> -ci<min> -cs<max> -fm` (MALVA:107) on the device: canonical ref_k-mers of the reads, a window with a byte outside
 * ACGT skipped (lower-case acgt count as upper case), a k-mer kept when seen >= min_count times (0 counts as 1), its count
 * capped at max_count.  Only the windows that pass the scan's own gate are counted: the others cannot change a counter
 * (BF::increment / KMAP::increment are no-ops for them, bloom_filter.hpp:100-113, kmap.hpp:114-122), so after mg_reads_finish
 * the counters are exactly what mg_kmc_scan_device leaves given KMC's table of the same reads -- record counters, lazy vectors
 * and groups alike.  Both filters must be finalised; ref_k <= MG_MAX_PACKED_K.
 *   mg_reads_begin       starts a count.  Keeps only the keys whose hash % n_parts == part: with N devices, every device sees
 *                        every chunk with part = its rank, n_parts = N, and the exchange (mg_counters_allreduce*) sums the
 *                        counters -- a k-mer's count is then global before min_count applies.
 *   mg_reads_add         a chunk of WHOLE records, one byte outside ACGT (e.g. '\n') between two of them: no window crosses it.
 *                        Returns once the bytes are up (pinned buffers from mg_host_alloc make that a DMA); the device packs
 *                        the chunk (2 bits + 1 mask bit per base) and keeps it until mg_reads_finish.
 *   mg_reads_add_device  the same from a device buffer, asynchronously: the context's stream reads the buffer (packed in place
 *                        when 4-byte aligned, else copied into a staging slot first), so the caller orders its writes to it
 *                        before the call (e.g. a device synchronize, or work on the context's stream) and leaves it unchanged
 *                        until mg_reads_finish (or mg_synchronize) returns.
 *   mg_reads_finish      count (passes whose pairs fit option reads_budget_mb, at least reads_passes of them), apply
 *                        min / max, scan the kept rows; *n_kept_out = rows kept.
 *   mg_reads_export      the kept rows (any order; only the gate's survivors, a subset of KMC's table): up to cap of them,
 *                        *n_out = all of them.
 *   mg_reads_stats       ms_out[5]: device milliseconds (HIP events) of pack, window + filter, file, reduce, scan;
 *                        counts_out[5]: bases, windows inside ACGT, gate survivors, passes, rows kept. */
int mg_reads_begin(mg_ctx *ctx, uint32_t min_count, uint32_t max_count, uint32_t part, uint32_t n_parts);
int mg_reads_add(mg_ctx *ctx, const char *seq, size_t bytes);
int mg_reads_add_device(mg_ctx *ctx, const void *d_seq, size_t bytes);
int mg_reads_finish(mg_ctx *ctx, uint64_t *n_kept_out);
int mg_reads_export(mg_ctx *ctx, uint64_t *hi, uint64_t *lo, uint32_t *cnt, size_t cap, uint64_t *n_out);
int mg_reads_stats(mg_ctx *ctx, float *ms_out, uint64_t *counts_out);

/* ---- cohort mode: several samples against one resident index ----------------
 * The reference genotypes one individual per run: every sample is a whole call_main (main.cpp:421-594) that loads the
 * index, parses the panel and cuts the blocks again before the one thing that differs happens -- the KMC scan
 * (main.cpp:482-500) and the counter lookups of set_coverages (main.cpp:151-184).  It has no counterpart for what follows.
 * In cohort mode a context holds the counters of n_planes samples (1..64) at once, sample-minor: the cell of filter
 * counter r, plane s at counts[r * G' + s], of exact-map key id at vals[id * G' + s], G' = n_planes rounded up to a power
 * of two (so the stride is a shift, and a counter's cells never straddle a 64-byte line they need not: 16 planes share one).
 *   mg_cohort_begin    both filters finalised, no multi-GPU group, no reads count open; allocates the planes, zeroed, and
 *                      selects plane 0.  The single-sample vectors are kept aside.  While the mode lasts the counters live in
 *                      the vectors alone (as on a context in a group: the records' own copies are not used), and the calls that
 *                      change the index (inserts, finalize, imports of filters / map, mg_index_*, mg_ref_scan*),
 *                      mg_counters_view and every mg_comm_* / mg_counters_allreduce* return MG_ERR_STATE.
 *   mg_cohort_select   the plane that scans (mg_kmc_scan*, mg_reads_*), per-k-mer increments and reads (mg_bf_increment,
 *                      mg_bf_get_count, mg_map_*, mg_lookup_cover, mg_call_isolated*, mg_cover_blocks*), mg_counters_reset /
 *                      _export_device / _import_device and the counter halves of mg_bf_export / mg_map_export act on.
 *                      Not between mg_reads_begin and mg_reads_finish.
 *   mg_cohort_end      frees the planes; the single-sample vectors are back, zeroed, and the next scan republishes the
 *                      records' copies.
 *   mg_cohort_info     n_planes (0 outside cohort mode) and the selected plane. */
int mg_cohort_begin(mg_ctx *ctx, uint32_t n_planes);
int mg_cohort_select(mg_ctx *ctx, uint32_t plane);
int mg_cohort_end(mg_ctx *ctx);
int mg_cohort_info(mg_ctx *ctx, uint32_t *n_planes, uint32_t *selected);

/* ---- multi-GPU exchange step --------------------------------------------- */

/* The scan's only state is two commutative wrapping-u32 sums:
 * [ bf counters (n_bf u32, in rank order) | map counters (n_map u32, in key
 * insertion order) ].  Ranks that built the same index agree on this layout,
 * so one sum all-reduce of this vector combines shard scans. */
int mg_counters_size(mg_ctx *ctx, uint64_t *n_bf, uint64_t *n_map);
int mg_counters_export_device(mg_ctx *ctx, void *d_u32_out);
int mg_counters_import_device(mg_ctx *ctx, const void *d_u32_in);
int mg_counters_reset(mg_ctx *ctx);
/* Zero-copy form: makes the two counter arrays one contiguous device allocation and returns
 * it (valid until the next insert / finalize / import).  An in-place all-reduce over
 * d_ptr[0 .. n_bf + n_map) replaces export + all-reduce + import. */
int mg_counters_view(mg_ctx *ctx, void **d_ptr, uint64_t *n_bf, uint64_t *n_map);

/* The exchange itself, inside the library: RCCL (librccl.so.1, opened on first use) over xGMI.  The reference has
 * no counterpart (single-threaded, CMakeLists.txt:46 links pthread and never uses it); SURVEY 8(b)/(e) define it.
 *
 *   one process per GPU   rank 0: mg_comm_unique_id(id); ship the 128 bytes to the other ranks (any channel);
 *                         every rank: mg_comm_init(ctx, rank, world, id); after its shard's mg_kmc_scan*:
 *                         mg_counters_allreduce(ctx) -- ncclAllReduce(sum, uint32), in place over the
 *                         mg_counters_view allocation, asynchronous on the context's stream.
 *   one process, N GPUs   mg_comm_init_all(ctxs, N) (one context per device) and, after the N shard scans,
 *                         mg_counters_allreduce_all(ctxs, N): the same all-reduces as one RCCL group.
 *                         Contexts that all sit on ONE device (rehearsing the N-way layout on a one-GPU box; RCCL
 *                         rejects duplicate devices) are summed by a kernel instead; mg_comm_info tells which.
 * Every rank must hold the same index (same inserts / same index file): the counter layout is then identical. */
#define MG_COMM_ID_BYTES 128
#define MG_COMM_NONE 0
#define MG_COMM_RCCL 1
#define MG_COMM_LOCAL 2
int mg_comm_unique_id(void *id_out /* MG_COMM_ID_BYTES */);
int mg_comm_init(mg_ctx *ctx, int rank, int world, const void *id);
int mg_comm_init_all(mg_ctx **ctxs, int n);
int mg_comm_destroy(mg_ctx *ctx);
int mg_comm_info(mg_ctx *ctx, int *rank, int *world, int *backend);
int mg_counters_allreduce(mg_ctx *ctx);
int mg_counters_allreduce_all(mg_ctx **ctxs, int n);
/* Two refinements of the exchange, both inside the library:
 *   the 16-bit packed form   two counters per 32-bit word on the links when that is exact, i.e. when no rank's partial counter
 *       exceeds 65535 / world (checked first: a max over the vector, then over the ranks; the plain 32-bit sum runs otherwise).
 *       Option exchange_pack: 0 never, 1 (default) for vectors of exchange_pack_min_mb (32) megabytes and more, 2 always.
 *       The call then waits for the guard's answer on the host; mg_get_option("exchange_packed") tells which form ran.
 *   _begin / _end   the same exchange on a stream of its own: _begin orders it behind what the context's stream holds (the
 *       scan), _end makes the context's stream wait for it; in between the caller may enqueue what needs no counters (the
 *       record loop's block cut, mg_cut_blocks_device), which then runs beside the collective.  main.cpp has neither: its
 *       loop B starts when loop A has ended (main.cpp:500-522).
 * mg_exchange_stats: duration of the context's most recent exchange (collective + pack / unpack, HIP events on its stream). */
int mg_counters_allreduce_begin(mg_ctx *ctx);
int mg_counters_allreduce_end(mg_ctx *ctx);
int mg_exchange_stats(mg_ctx *ctx, float *ms_out, int *packed_out);

/* ---- per-variant path ----------------------------------------------------- */

/* set_coverages (main.cpp:151-184) over flat signature descriptors of any
 * number of blocks: allele slot a owns signatures [allele_sig_off[a],
 * allele_sig_off[a+1]); signature s owns rows [sig_kmer_off[s], sig_kmer_off[s+1]);
 * is_ref[row] != 0 -> KMAP::get_count, else BF(bf)::get_count.
 * cov_out[a] = max over signatures of the truncating running mean. */
int mg_lookup_cover(mg_ctx *ctx, const char *rows, size_t stride, size_t n_rows, const uint8_t *is_ref,
                    const uint64_t *sig_kmer_off, size_t n_sigs, const uint64_t *allele_sig_off, size_t n_alleles,
                    uint32_t *cov_out);

/* Block cutting of the record loops (main.cpp:341, 547: `!vb.is_near_to_last(v) || last_seq_name != v.seq_name`, with
 * VB::is_near_to_last = are_near(last variant, v), var_block.hpp:77-80, 417-423 -- in the reference's float arithmetic) for
 * a batch of n_vars KEPT records in file order, on the device.  contig_id[i] identifies record i's sequence; give
 * contig_id[0] the id of `last_seq_name` as it stands when record 0 arrives (the name of the file's first record, kept or
 * not, for the first batch; the previous kept record's name afterwards) and put the previous batch's last record in front
 * as record 0 to continue a block across batches.  blk_var_off_out (n_vars + 1 entries) receives the first record of
 * every block and n_vars behind the last; these are the blk_var_off of mg_cover_blocks / mg_index_blocks. */
int mg_cut_blocks(mg_ctx *ctx, size_t n_vars, const int32_t *pos, const uint32_t *ref_size, const uint32_t *min_size,
                  const uint32_t *contig_id, uint32_t *blk_var_off_out, size_t *n_blocks_out);

/* A batch of blocks of any shape in HOST memory, as the three host forms of the record loop below take it (mg_panel_dev is the
 * same panel resident on the device).  Variants are flat across blocks; every pointer is a HOST pointer. */
typedef struct mg_blocks_host {
    size_t n_blocks;
    const uint64_t *blk_ref_base;    /* [n_blocks] where the block's contig starts in the uploaded reference ... */
    const uint32_t *blk_ref_len;     /* [n_blocks] ... and how long it is */
    const uint32_t *blk_var_off;     /* [n_blocks + 1] first record of every block, n_vars behind the last (mg_cut_blocks) */
    size_t n_vars;
    const int32_t *pos;              /* [n_vars] 0-based position in the block's contig (Variant::ref_pos) */
    const uint32_t *ref_size;        /* [n_vars] */
    const uint32_t *min_size;        /* [n_vars] */
    const uint8_t *present;          /* [n_vars] Variant::is_present */
    const uint32_t *var_allele_off;  /* [n_vars + 1]; slots = var_allele_off[n_vars], one per (variant, allele) */
    const uint32_t *allele_off;      /* [slots + 1] into pool */
    const char *pool;                /* [pool_len] the alleles' text */
    size_t pool_len;
    const uint8_t *canon;            /* [slots] first allele index of the variant with the same text (variant.hpp:228) */
    uint32_t n_samples;              /* kept panel samples */
    /* gt[v * n_samples + s] = a1 | a2 << 7 | phased << 14 (variant.hpp:158-211); a1 and a2 are below the record's allele count (the
     * reference reads out of bounds otherwise; the library does not check: its caller's reader does) */
    const uint16_t *gt;              /* [n_vars][n_samples], or NULL with the sparse form */
    /* the sparse form of mg_panel_dev (only the samples whose genotype word is not sp_default: what crosses PCIe for a 27,934-sample
     * panel drops from 56 KB per record to a few bytes per non-reference genotype).  Given (non-NULL sp_off), `gt` is ignored; both
     * NULL with n_samples > 0 is MG_ERR_ARG. */
    const uint32_t *sp_off;          /* [n_vars + 1] or NULL */
    const uint32_t *sp_sample;       /* [sp_off[n_vars]] ascending below n_samples inside a record */
    const uint16_t *sp_gt;           /* [sp_off[n_vars]] */
    uint16_t sp_default;
} mg_blocks_host;

/* VB::extract_kmers (var_block.hpp:95-219, chains :436-677, haplotype picks :709-786) fused with
 * set_coverages (main.cpp:151-184) for blocks of any shape, enumerated ON THE DEVICE.  cov_out as in mg_lookup_cover, one
 * slot per (variant, allele).  overflow_out[v] = 1 where a fixed device capacity (16 chains per side, 32 members per
 * chain side, 14 unphased members, 127 alleles, k <= 64) or a window clipped by a contig end was hit: redo
 * that variant's block through the host enumerator + mg_lookup_cover.  A NULL batch is MG_ERR_ARG. */
int mg_cover_blocks(mg_ctx *ctx, const mg_blocks_host *blocks, int haploid, uint32_t *cov_out, uint8_t *overflow_out);

/* The same enumeration at INDEX time: VB::extract_kmers + add_kmers_to_bf (main.cpp:349-350, 122-144) for blocks of any
 * shape -- every signature k-mer of allele 0 is added to the exact map (KMAP::add_key), every other one sets its bit of
 * `bf` (BF::add_key).  The batch as for mg_cover_blocks (the panel genotypes decide which alleles have signatures); the
 * blocks hold only the variants `index` keeps (has_alts and is_present, main.cpp:332).  overflow_out[v] = 1: nothing of
 * that variant was inserted (a device capacity, a window clipped by a contig end, or a REF k-mer the packed table cannot
 * hold) -- enumerate its block on the host and insert with mg_map_insert / mg_bf_insert.  Before mg_bf_finalize.
 * Counter ids of keys inserted here follow the order the device reached them in; ranks of a multi-GPU call agree on
 * the layout by loading the same index file. */
int mg_index_blocks(mg_ctx *ctx, const mg_blocks_host *blocks, int haploid, uint8_t *overflow_out);

/* ---- the record loop on a RESIDENT panel (main.cpp:522-579 / 309-370 with every array already in HBM) --------------------
 * A panel is the kept records of a VCF (or of a batch of one) in file order, as flat arrays: every pointer below is a
 * DEVICE pointer on the context's GPU, nothing is copied or re-uploaded, and the calls are asynchronous on the
 * context's stream (mg_index_blocks_device excepted, see there).  Record v sits on sequence contig_id[v], which starts
 * at contig_base[] in the buffer of mg_reference_upload and is contig_len[] long; the other arrays are those of
 * mg_blocks_host.  One step of `call` on a resident panel is
 *     mg_cut_blocks_device -> mg_cover_blocks_device -> mg_genotype_device
 * and of `index`:  mg_cut_blocks_device -> mg_index_blocks_device. */
typedef struct mg_panel_dev {
    uint64_t n_vars;
    uint32_t n_contigs;
    uint32_t n_samples;
    const uint64_t *contig_base;     /* [n_contigs] */
    const uint32_t *contig_len;      /* [n_contigs] */
    const uint32_t *contig_id;       /* [n_vars]; contig_id[0] as for mg_cut_blocks */
    const int32_t *pos;              /* [n_vars] Variant::ref_pos */
    const uint32_t *ref_size;        /* [n_vars] */
    const uint32_t *min_size;        /* [n_vars] */
    const uint8_t *present;          /* [n_vars] Variant::is_present */
    const uint32_t *var_allele_off;  /* [n_vars + 1] */
    const uint32_t *allele_off;      /* [slots + 1] */
    const char *pool;
    const uint8_t *canon;            /* [slots] */
    const uint16_t *gt;              /* [n_vars][n_samples] -- or NULL with the sparse form below */
    /* sparse genotypes (a panel of tens of thousands of samples is nearly all 0|0): record v's entries are
     * [sp_off[v], sp_off[v + 1]) of sp_sample (ascending sample numbers) / sp_gt (their genotype words); every sample
     * without an entry carries the word sp_default (1 << 14 = 0|0 phased for a phased panel, 0 = 0/0 for an unphased one:
     * the phase bit of a homozygous genotype still decides how its sample's OTHER genotypes along a chain combine,
     * var_block.hpp:758-782, so it is part of the word).  Given (non-NULL sp_off), `gt` is ignored. */
    const uint32_t *sp_off;          /* [n_vars + 1] or NULL */
    const uint32_t *sp_sample;
    const uint16_t *sp_gt;
    uint32_t sp_default;
    /* bytes of `pool` (= allele_off[last allele slot]).  Given (non-zero, and `pool` 4-byte aligned) the record loop packs the
     * alleles to 2 bits per base at the start of every call and assembles signature k-mers from the packed form; 0: from the bytes. */
    uint64_t pool_bytes;
} mg_panel_dev;
/* The cut (main.cpp:341, 547) of all n_vars records: d_blk_var_off_out ([n_vars + 1] u32), d_n_blocks_out (one u64), and
 * -- optional, NULL to skip -- d_var_block_out ([n_vars] u32: the block of every record, which the two calls below
 * otherwise derive again).  Needs contig_id, pos, ref_size, min_size only. */
int mg_cut_blocks_device(mg_ctx *ctx, const mg_panel_dev *panel, void *d_blk_var_off_out, void *d_var_block_out, void *d_n_blocks_out);
/* extract_kmers + set_coverages (main.cpp:556-557) for every block: d_cov_out ([slots] u32) and d_overflow_out ([n_vars]
 * u8) as mg_cover_blocks returns them.  A block is evaluated against the sequence of its first record (`last_seq_name` at
 * the flush, main.cpp:556).  Three tiers (csrc/block_pipeline.h): blocks of one variant whose alleles are all shorter than k
 * take the fused lone-variant lookup of mg_call_isolated; the other records a pipeline of flat kernels (one thread per record
 * for the chain walks, one wave per chain for the distinct haplotype picks, one thread per signature k-mer); what exceeds
 * that pipeline's capacities the workgroup-per-record kernel; what exceeds ITS capacities is flagged in d_overflow_out. */
int mg_cover_blocks_device(mg_ctx *ctx, const mg_panel_dev *panel, const void *d_blk_var_off, const void *d_var_block /* or NULL */,
                           const void *d_n_blocks, int haploid, void *d_cov_out, void *d_overflow_out);
/* mg_cover_blocks_device for every plane of a context in cohort mode (the record loop of main.cpp:522-579, which the
 * reference repeats per sample inside call_main, main.cpp:421-594): d_cov_out is [n_planes][slots] u32, plane-major
 * (slots = var_allele_off[n_vars]); plane s holds exactly what mg_cover_blocks_device writes with plane s selected.
 * d_overflow_out ([n_vars] u8) does not depend on the sample.  Tier 1 runs ONCE for all planes: classification, signature
 * k-mer, hash and the walk to the record once per allele, then the record's n_planes cells -- one contiguous run -- become
 * the n_planes coverages.  Tiers 2 and 3 run plane by plane over the general list tier 1 wrote once.  The selected plane
 * is left as it was.  Reads var_allele_off[n_vars] back (waits for the stream once, on four bytes), asynchronous otherwise.
 * mg_cohort_stats (waits for it): ms_out[0] tier 1 over all planes, ms_out[1] tiers 2 and 3 of all planes (mg_blocks_stats describes
 * the single-sample call only and returns MG_ERR_STATE after this one). */
int mg_cover_blocks_cohort_device(mg_ctx *ctx, const mg_panel_dev *panel, const void *d_blk_var_off, const void *d_var_block /* or NULL */,
                                  const void *d_n_blocks, int haploid, void *d_cov_out, void *d_overflow_out);
int mg_cohort_stats(mg_ctx *ctx, float *ms_out);
/* The host form (as mg_cover_blocks is of mg_cover_blocks_device): the batch is uploaded ONCE and covered for every plane; cov_out is
 * [n_planes][slots], overflow_out [n_vars].  Knows the slot count from var_allele_off, so it does not wait for the device before the
 * copy back.  Synchronous. */
int mg_cover_blocks_cohort(mg_ctx *ctx, const mg_blocks_host *blocks, int haploid, uint32_t *cov_out /* [n_planes][slots] */, uint8_t *overflow_out);
/* extract_kmers + add_kmers_to_bf (main.cpp:349-350) for every block (the panel holds only what `index` keeps,
 * main.cpp:332); d_overflow_out as mg_index_blocks.  The arrays stay where they are, but the call waits for the device
 * twice on eight bytes: the exact map is sized from a counting pass before the insert pass runs. */
int mg_index_blocks_device(mg_ctx *ctx, const mg_panel_dev *panel, const void *d_blk_var_off, const void *d_var_block /* or NULL */,
                           const void *d_n_blocks, int haploid, void *d_overflow_out);

/* Panel genotypes straight from VCF text: Variant::extract_genotypes (variant.hpp:158-211) over the sample columns of a batch
 * of records, decoded on the device into the sparse form of mg_panel_dev.  The host finds each record's ninth tab and the
 * position of GT in its FORMAT column and parses nothing else of the sample columns.
 *   text, text_bytes      host buffer holding the records' lines (only the range the spans cover is uploaded)
 *   span_off/span_len[r]  record r's sample columns: from the byte after the FORMAT column's tab to the end of the line
 *                         (terminator excluded); length 0 = the record has no sample columns (every kept sample reads ".")
 *   gt_index[r]           position of GT among the ':'-separated FORMAT keys (the caller has checked that it is there)
 *   n_columns, keep       sample columns of the header; keep[i] != 0: column i is one of the kept samples (-s), NULL = all
 * Out, per record: sp_off[n_records + 1] (entries of record r at [sp_off[r], sp_off[r + 1])), raw_mask (bit a: raw allele
 * number a, mod 64, occurs in a kept sample -- both alleles unless haploid), max_allele (the largest allele number: the
 * caller checks it against the record's allele count as variant.hpp would crash on it, and decodes a record with a number
 * above 127 itself, whose words here are truncated).  *sp_default = the word of the samples without an entry (0|0 phased or
 * 0/0, whichever the batch holds more of), *n_entries = sp_off[n_records].  The entries themselves stay on the device until
 * mg_decode_gt_entries copies them out (sample numbers count KEPT samples, ascending inside a record).  Synchronous. */
int mg_decode_gt_text(mg_ctx *ctx, const char *text, size_t text_bytes, size_t n_records, const uint64_t *span_off, const uint32_t *span_len,
                      const int32_t *gt_index, uint32_t n_columns, const uint8_t *keep, int haploid, uint16_t *sp_default, uint32_t *sp_off,
                      uint64_t *raw_mask, uint32_t *max_allele, uint64_t *n_entries);
int mg_decode_gt_entries(mg_ctx *ctx, uint32_t *sp_sample, uint16_t *sp_gt);

/* Result codes of mg_genotype / mg_call_isolated per variant */
#define MG_GT_NORMAL 0   /* likelihood list computed                              */
#define MG_GT_OVERCOV 1  /* some allele > max_cov: (best_geno,0) per such allele  */
#define MG_GT_SINGLE 2   /* one allele only: (best_geno,1)                        */
#define MG_GT_NOCOV 3    /* all coverages 0: (best_geno,0)                        */

/* Index-time counterpart of mg_call_isolated for blocks of ONE variant whose alleles are all shorter than k: VB::extract_kmers
 * with comb = {v} (var_block.hpp:95-219) + add_kmers_to_bf (main.cpp:122-144) on the device -- allele 0's signature k-mer goes
 * into the exact map (KMAP::add_key), the signature of every other allele some panel haplotype carries (present_mask) sets its
 * bit of `bf` (BF::add_key).  pos, offsets, pool, present_mask and flags as for mg_call_isolated (flags bit0: is_present and
 * not within k of a contig end, var_block.hpp:104; flanks inside the contig).  overflow_out[v] = 1: nothing of that variant
 * was inserted (a base outside ACGT in its window or alleles, more than 64 alleles, k outside 17..64) -- enumerate it on the
 * host and insert with mg_map_insert / mg_bf_insert.  Before mg_bf_finalize; after mg_reference_upload.  Variant v's REF key
 * takes insertion row (rows so far) + v; the index FILE fixes the counter layout for every GPU of a call. */
int mg_index_isolated(mg_ctx *ctx, size_t n_vars, const uint64_t *pos, const uint32_t *var_allele_off, const uint32_t *allele_off,
                      const char *allele_pool, size_t pool_len, const uint64_t *present_mask, const uint8_t *flags,
                      uint8_t *overflow_out);

/* VB::genotype (var_block.hpp:224-330) + the normalise / first-strict-max / GQ
 * part of VB::output_variants (:366-394).  Variant v owns allele slots
 * [var_allele_off[v], var_allele_off[v+1]).  gt2 = -1 in haploid mode.
 * probs (optional, may be NULL): normalised list in the reference's order,
 * variant v at var_gt_off[v] (caller-provided offsets, A or A(A+1)/2 each). */
int mg_genotype(mg_ctx *ctx, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off, size_t n_vars,
                float error_rate, int max_cov, int haploid, int32_t *gt1, int32_t *gt2, int32_t *gq,
                uint8_t *status, double *probs, const uint64_t *var_gt_off);
/* same, every array already resident on the device (asynchronous) */
int mg_genotype_device(mg_ctx *ctx, const void *d_cov, const void *d_freq, const void *d_var_allele_off, size_t n_vars,
                       float error_rate, int max_cov, int haploid, void *d_gt1, void *d_gt2, void *d_gq, void *d_status,
                       void *d_probs, const void *d_var_gt_off);

/* Fused device path for blocks that hold ONE variant whose alleles are all
 * shorter than k (the isolated-SNP/indel case): signature enumeration
 * (var_block.hpp:95-219 with comb = {v}), lookup + coverage, likelihoods and
 * GT/GQ in one launch.  `reference` is the concatenation of the upper-cased
 * contigs already uploaded with mg_reference_upload; pos[v] is the variant's
 * offset in that buffer.  flags bit0: eligible (is_present and not within k of
 * a contig end, var_block.hpp:104).  An eligible variant's flanks -- k/2 bases
 * before pos, ceil(k/2) after the REF allele -- must lie inside its contig: a
 * right flank clipped by the contig end makes a shorter k-mer in the reference
 * (var_block.hpp:187), which is mg_cover_blocks' / the host enumerator's case.  present_mask bit a: some panel haplotype
 * carries allele a (build_alleles_combs, var_block.hpp:734-786).  probs (optional):
 * normalised likelihood lists at caller-provided var_gt_off, as in mg_genotype. */
int mg_reference_upload(mg_ctx *ctx, const char *ascii, size_t len);
int mg_reference_upload_device(mg_ctx *ctx, const void *d_ascii, size_t len); /* from a device buffer (copied) */
int mg_call_isolated(mg_ctx *ctx, size_t n_vars, const uint64_t *pos, const uint32_t *var_allele_off,
                     const uint32_t *allele_off, const char *allele_pool, size_t pool_len, const float *freq,
                     const uint64_t *present_mask, const uint8_t *flags, float error_rate, int max_cov, int haploid,
                     uint32_t *cov_out, int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status, double *probs,
                     const uint64_t *var_gt_off);
/* same, every array already resident on the device (asynchronous).  d_probs / d_var_gt_off
 * (both or neither; as in mg_genotype) double as the workspace that saves recomputing
 * each likelihood for the normalisation pass. */
int mg_call_isolated_device(mg_ctx *ctx, size_t n_vars, const void *d_pos, const void *d_var_allele_off,
                            const void *d_allele_off, const void *d_allele_pool, const void *d_freq,
                            const void *d_present_mask, const void *d_flags, float error_rate, int max_cov,
                            int haploid, void *d_cov_out, void *d_gt1, void *d_gt2, void *d_gq, void *d_status,
                            void *d_probs, const void *d_var_gt_off);

/* ---- the sample columns of a multi-sample VCF ------------------------------------
 * mg_cells: the cells of a batch, as the encoders of this section and of the BCF section below take them.  Pointer members hold host
 * pointers in a host form and device pointers in a _device form.  `fields` says which optional FORMAT fields are made; an array
 * whose bit is not set is not read and may be NULL.
 *   always        gt1 / gt2 / gq: [n_planes][n_vars] int32, plane-major, as n_planes calls of mg_genotype / mg_call_isolated fill them
 *                 (n_planes 1..64; gt2 is not read in haploid mode and may then be NULL).  use_mask != 0: a cell whose gq < min_gq has
 *                 its genotype made missing and keeps every other field.  cov ([n_planes][slots] uint32, slots =
 *                 var_allele_off[n_vars]) is optional and adds the field COVS; var_allele_off is [n_vars + 1] uint32.  With neither
 *                 bit set, cov and var_allele_off are given both or neither.  allele_class is not read by an encoder.
 *   MG_CELLS_GP   the field GP behind GT, GQ and COVS.  Requires var_allele_off and var_gt_off ([n_vars + 1] uint64) with or without
 *                 cov, and with n_vars > 0 probs and status.  The values are the doubles mg_genotype / mg_call_isolated leave in
 *                 probs (gt.second / total_qual, var_block.hpp:381: the numbers behind GTS= of the single-sample output): probs is
 *                 [n_planes][var_gt_off[n_vars]], record v's values of plane p start at probs[p * var_gt_off[n_vars] +
 *                 var_gt_off[v]]; status is [n_planes][n_vars] uint8.  The record has A = var_allele_off[v + 1] - var_allele_off[v]
 *                 alleles and G = A (haploid) or A (A + 1) / 2 genotypes.  probs holds them in the reference's order -- a outer,
 *                 c >= a inner: 0/0, 0/1, 0/2, 1/1, .. -- and GP is in VCF order, genotype j/k (j <= k) at index k (k + 1) / 2 + j:
 *                 0/0, 0/1, 1/1, 0/2, ..; haploid: the index is the allele.  A cell whose status is not MG_GT_NORMAL has no GP and
 *                 its probs are not read.  A value is PRINTABLE when its sign bit is clear and 0 <= p <= 1 -- NaN, -0.0,
 *                 negatives, anything above 1 and the infinities are not.
 *   MG_CELLS_PL   the field PL behind the cell's last.  Requires var_allele_off, var_gt_off and, with n_vars > 0, pl:
 *                 [n_planes][var_gt_off[n_vars]] int32, a record's G values ALREADY in VCF order (what mg_phred_likelihoods leaves;
 *                 the encoder copies and does not permute).  probs and status are given both or neither (and both with
 *                 MG_CELLS_GP).  The encoder does not know where the integers came from: any int32 is a value, MG_PL_MISSING alone
 *                 is special.  A masked cell keeps its PL.
 * mg_format_calls: the GT/GQ print of VB::output_variants (var_block.hpp:337-396), which the reference does for its one individual,
 * repeated per sample: the reference has no multi-sample output.  The context need not be in cohort mode: the call formats arrays
 * and reads no counters.  Row v is text_out[row_off_out[v] .. row_off_out[v + 1]): for every plane in order a tab and the cell,
 * then '\n'.  The cell is `GT:GQ[:COVS][:GP][:PL]`.  GT is `<gt1>` in haploid mode, else `<gt1>/<gt2>`, under the mask `.` or `./.`;
 * COVS the record's coverages of that plane, comma-separated.  Every integer prints as std::to_string(int) prints it, a coverage as
 * std::to_string((int)cov).  GP is the G comma-separated values (none for a record without alleles), or one `.` for a cell that is
 * not MG_GT_NORMAL; a printable value prints exactly as printf("%f") prints it, always 8 bytes, `0.dddddd` or `1.000000`: rounded to
 * nearest on the exact binary value, ties to even, as glibc does, in integers (N = m 10^6 with m the 53-bit significand, q = N >> s,
 * s = 1075 - the biased exponent, and the remainder against 2^(s-1)); an unprintable one prints `.`.  PL is the G comma-separated
 * values, MG_PL_MISSING as `.`; the whole field is one `.` when G == 0 or every value of the cell is missing.
 * n_vars == 0 is legal: row_off_out[0] = 0.  *text_bytes_out always receives the bytes the text needs; when that is more
 * than text_cap the call returns MG_ERR_LIMIT, nothing is written at or behind text_cap, the text_cap bytes in front of it are the
 * text's first text_cap bytes, row_off_out is valid all the same, and the caller may come again with a larger buffer.  A NULL
 * cells pointer: MG_ERR_ARG.  The host form synchronises; the device form is asynchronous on the context's stream until it reads the
 * 8-byte total back (text_bytes_out is a HOST pointer in both).
 * mg_format_stats (waits for it): ms_out[3], device milliseconds of the most recent call's length pass, scan and write pass. */
#define MG_CELLS_GP 1u
#define MG_CELLS_PL 2u
#define MG_PL_MISSING INT32_MIN
typedef struct mg_cells {
    size_t n_vars;
    uint32_t n_planes;
    int haploid;
    const void *gt1, *gt2, *gq;
    int use_mask;
    int32_t min_gq;
    const void *cov, *var_allele_off;
    const void *probs, *var_gt_off, *status, *pl;
    const void *allele_class; /* mg_sample_counts' own; no encoder reads it */
    uint32_t fields;          /* MG_CELLS_GP | MG_CELLS_PL */
} mg_cells;
int mg_format_calls(mg_ctx *ctx, const mg_cells *cells, char *text_out, size_t text_cap, uint64_t *row_off_out, uint64_t *text_bytes_out);
int mg_format_calls_device(mg_ctx *ctx, const mg_cells *cells, void *d_text_out, size_t text_cap, void *d_row_off_out, uint64_t *text_bytes_out);
int mg_format_stats(mg_ctx *ctx, float *ms_out);

/* ---- the site tags of a multi-sample VCF (AC / AN / AF / NS) -----------------------
 * mg_site_counts: the allele counts of every record over the planes.  gt1 / gt2 / gq as for mg_format_calls (n_planes 1..64;
 * gt2 is not read in haploid mode, gq not unless use_mask).  A cell is CALLED unless use_mask != 0 and its gq < min_gq.  Record v
 * owns the slots ac[var_allele_off[v] .. var_allele_off[v + 1]), one per allele, REF first: a called cell adds 1 to slot gt1 and,
 * in diploid mode, 1 to slot gt2; an allele index outside the record's slots (a negative one included) is not counted and
 * nothing is written outside the record's slots.  ns[v] receives the number of planes whose cell is called.  accumulate != 0
 * adds to what ac / ns hold (groups of a cohort larger than 64 are summed this way), accumulate == 0 overwrites.  The host
 * form synchronises; the device form is asynchronous on the context's stream.
 * mg_format_site_info: row v = text_out[row_off_out[v] .. row_off_out[v + 1]) is the INFO string of record v, no tab and no
 * newline: `AC=a1,a2,..;AN=n;AF=f1,f2,..;NS=s`.  AC_i is the record's slot i (i >= 1), AN the sum of all its slots, NS ns[v].
 * AF_i = AC_i / AN in integers: q = (2 * AC_i * 10^6 + AN) / (2 * AN) (64-bit; half rounds up at the sixth decimal); q == 0
 * prints `0`, q == 10^6 prints `1`, anything else `0.` and q as six zero-padded digits with trailing zeros removed; AN == 0
 * prints `.` for every AF.  A record with fewer than two slots prints `AN=n;NS=s`.  Buffer contract as mg_format_calls:
 * *text_bytes_out (a HOST pointer in both forms) always receives the bytes needed, MG_ERR_LIMIT when that exceeds text_cap,
 * nothing written at or behind text_cap, the bytes in front of it the text's first, row_off_out valid all the same.
 * mg_site_stats (waits): ms_out[2], device milliseconds of the most recent mg_site_counts* and of the most recent
 * mg_format_site_info* (its three passes together); 0 for a kind not called yet, MG_ERR_STATE when neither was. */
int mg_site_counts(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                   int32_t min_gq, const uint32_t *var_allele_off, int accumulate, uint32_t *ac, uint32_t *ns);
int mg_site_counts_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                          int32_t min_gq, const void *d_var_allele_off, int accumulate, void *d_ac, void *d_ns);
int mg_format_site_info(mg_ctx *ctx, size_t n_vars, const uint32_t *ac, const uint32_t *ns, const uint32_t *var_allele_off, char *text_out, size_t text_cap,
                        uint64_t *row_off_out, uint64_t *text_bytes_out);
int mg_format_site_info_device(mg_ctx *ctx, size_t n_vars, const void *d_ac, const void *d_ns, const void *d_var_allele_off, void *d_text_out, size_t text_cap,
                               void *d_row_off_out, uint64_t *text_bytes_out);
int mg_site_stats(mg_ctx *ctx, float *ms_out);

/* ---- the pair table of a multi-sample call set --------------------------------------
 * For every pair of planes (samples) and every record where both are called, the joint count of their genotypes: a 3 x 3 table
 * per pair, from which IBS0/1/2, discordance and a KING-style kinship follow.  There is no reference call to cite: the reference
 * genotypes one individual per run and has nothing that looks across samples.
 * mg_pack_dosage: the cells of a batch as bit planes.  gt1 / gt2 / gq, n_planes (1..64) and CALLED exactly as for mg_site_counts:
 * [n_planes][n_vars] int32, plane-major; gt2 is not read in haploid mode and may be NULL, gq not unless use_mask; a cell is called
 * unless use_mask != 0 and its gq < min_gq.  var_allele_off ([n_vars + 1]) is required.  planes_out is uint64_t
 * [n_planes][3][W], W = (n_vars + 63) / 64: bit v & 63 of word v >> 6 of planes_out[p][d] is set exactly when record v has two
 * alleles (var_allele_off[v + 1] - var_allele_off[v] == 2), the cell (p, v) is called, every allele index the mode reads is 0 or 1,
 * and the cell's dosage is d -- gt1 + gt2 in diploid mode, 2 * gt1 in haploid mode (the allele stands as a homozygote: class 1 is
 * empty).  Every other bit is 0, the bits of the last word at and beyond n_vars and every bit of a record that is not biallelic
 * included: a cell has at most one of its three bits set.  Every word of the output is written, the caller need not clear it;
 * n_vars == 0 is legal and writes nothing.  The host form synchronises; the device form is asynchronous on the context's stream.
 * mg_pair_counts: planes_a is [n_a][3][n_words], planes_b [n_b][3][n_words], as mg_pack_dosage lays them out (n_a, n_b 1..64).
 * counts is uint64_t [n_a][n_b][9]: counts[(i * n_b + j) * 9 + 3 * da + db] = the sum over w of
 * popcount(A[i][da][w] & B[j][db][w]).  planes_b == NULL: B is A, n_b must equal n_a, and the whole square is filled -- the
 * result is symmetric under swapping i, j and transposing the 3 x 3 table.  accumulate != 0 adds to what counts holds (the
 * batches of a pass, the groups of a cohort larger than 64 are summed this way); accumulate == 0 overwrites all n_a * n_b * 9
 * entries, so n_words == 0 then zeroes them.  n_a or n_b out of range, a NULL counts, a NULL planes_a with n_words > 0,
 * n_b != n_a with a NULL planes_b: MG_ERR_ARG.  The host form synchronises; the device form is asynchronous on the context's stream.
 * mg_pairs_stats (waits): ms_out[2], device milliseconds of the most recent mg_pack_dosage* and of the most recent
 * mg_pair_counts*; 0 for a kind not called yet, MG_ERR_STATE when neither was.
 * These calls keep their device copies and events apart from the encoders' and the site tags': a call of one kind between two of
 * another changes nothing in either. */
int mg_pack_dosage(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                   int32_t min_gq, const uint32_t *var_allele_off, uint64_t *planes_out);
int mg_pack_dosage_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                          int32_t min_gq, const void *d_var_allele_off, void *d_planes_out);
int mg_pair_counts(mg_ctx *ctx, size_t n_words, const uint64_t *planes_a, uint32_t n_a, const uint64_t *planes_b, uint32_t n_b, int accumulate,
                   uint64_t *counts);
int mg_pair_counts_device(mg_ctx *ctx, size_t n_words, const void *d_planes_a, uint32_t n_a, const void *d_planes_b, uint32_t n_b, int accumulate,
                          void *d_counts);
int mg_pairs_stats(mg_ctx *ctx, float *ms_out);

/* ---- the per-sample table of a multi-sample call set --------------------------------
 * For every plane (sample) the sums of its cells along the records: call rate, het / hom, Ts / Tv, the GQ sum and histogram, the
 * coverage and the genotyper's status codes follow from them.  mg_site_counts sums the cell matrix along the samples, per record;
 * this sums it along the records, per sample.  There is no reference call to cite: the reference genotypes one individual per run.
 * gt1 / gt2 / gq and n_planes (1..64) exactly as for mg_site_counts: [n_planes][n_vars] int32, plane-major; gt2 is not read in
 * haploid mode and may be NULL; gq is read always (the histogram).  status is [n_planes][n_vars] bytes, the MG_GT_* codes, or NULL:
 * the four status slots then stay untouched.  cov is [n_planes][slots] with slots = var_allele_off[n_vars], or NULL: COV_SUM then
 * stays untouched.  allele_class is [slots], one byte per allele slot -- 0 REF or none, 1 transition, 2 transversion, 3 insertion,
 * 4 deletion, 5 other; a record's slot 0 is not read -- or NULL: TS .. OTHER then stay untouched.  var_allele_off ([n_vars + 1]) is
 * required with n_vars > 0.  counts is uint64_t [n_planes][MG_SAMPLE_SLOTS].  With A = var_allele_off[v + 1] - var_allele_off[v],
 * a cell (p, v) counts as follows:
 *   RECORDS   every cell
 *   MASKED    use_mask != 0 and gq < min_gq, decided first
 *   BAD       not masked, and some allele index the mode reads is outside [0, A) (negative ones included)
 *   CALLED    neither masked nor bad: RECORDS = MASKED + BAD + CALLED
 *   HOM_REF   called, every index read is 0
 *   HET       called, diploid, gt1 != gt2
 *   HOM_ALT   called, gt1 != 0 and (haploid or gt1 == gt2)
 *   HET_ALT   called, diploid, gt1 != gt2, both nonzero (a subset of HET)
 *   TS TV INS DEL OTHER   called: for each DISTINCT nonzero allele index of the cell, 1 to the slot of
 *             allele_class[var_allele_off[v] + index] (class 0 or above 5: nothing)
 *   GQ_SUM    called: gq as a signed 64-bit value, added in two's complement
 *   COV_SUM   every cell, masked ones included: the sum of the record's A coverages of that plane
 *   ST_NORMAL ST_OVERCOV ST_SINGLE ST_NOCOV   every cell, by status; any other code: nothing
 *   GQ_0 .. GQ_90   every cell that is not BAD, masked ones included: bin min(max(gq, 0), 99) / 10
 * Slots 29..31 are reserved: written as 0 without accumulate, left alone with it.  accumulate != 0 adds to what counts holds (the
 * batches of a pass are summed this way); accumulate == 0 overwrites all n_planes * MG_SAMPLE_SLOTS entries, so n_vars == 0 then
 * zeroes them.  The sums are integers: the result does not depend on how the records are cut into calls.  n_planes out of
 * range, a NULL counts, a NULL gt1 / gq / var_allele_off with n_vars > 0, a NULL gt2 in diploid mode: MG_ERR_ARG.  The host form
 * synchronises; the device form (every array a device pointer) is asynchronous on the context's stream.
 * mg_sample_stats (waits): ms_out[1], device milliseconds of the most recent mg_sample_counts*; MG_ERR_STATE before the first.
 * The calls keep their device copies and their events apart from the encoders', the site tags' and the pair table's. */
#define MG_SAMPLE_SLOTS 32
#define MG_SS_RECORDS 0
#define MG_SS_MASKED 1
#define MG_SS_BAD 2
#define MG_SS_CALLED 3
#define MG_SS_HOM_REF 4
#define MG_SS_HET 5
#define MG_SS_HOM_ALT 6
#define MG_SS_HET_ALT 7
#define MG_SS_TS 8
#define MG_SS_TV 9
#define MG_SS_INS 10
#define MG_SS_DEL 11
#define MG_SS_OTHER 12
#define MG_SS_GQ_SUM 13
#define MG_SS_COV_SUM 14
#define MG_SS_ST_NORMAL 15
#define MG_SS_ST_OVERCOV 16
#define MG_SS_ST_SINGLE 17
#define MG_SS_ST_NOCOV 18
#define MG_SS_GQ_0 19      /* .. MG_SS_GQ_0 + 9: GQ 90 and above */
#define MG_SS_COUNTED 29   /* the slots in use; the rest is reserved */
int mg_sample_counts(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                     int32_t min_gq, const uint8_t *status, const uint32_t *cov, const uint32_t *var_allele_off, const uint8_t *allele_class, int accumulate,
                     uint64_t *counts);
int mg_sample_counts_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                            int32_t min_gq, const void *d_status, const void *d_cov, const void *d_var_allele_off, const void *d_allele_class, int accumulate,
                            void *d_counts);
int mg_sample_stats(mg_ctx *ctx, float *ms_out);

/* ---- the per-record table of a multi-sample call set --------------------------------
 * For every record and allele the genotype counts over the planes, and for every (record, ALT) the exact test of Hardy-Weinberg
 * proportions that follows from them.  There is no reference call to cite: the reference genotypes one individual per run.
 * mg_site_geno_counts: gt1 / gt2 / gq, n_planes (1..64), use_mask / min_gq, var_allele_off and accumulate exactly as for
 * mg_site_counts: [n_planes][n_vars] int32, plane-major; gt2 is not read in haploid mode and may be NULL, gq not unless use_mask.
 * With A = var_allele_off[v + 1] - var_allele_off[v], a cell of record v is USABLE when it is not masked (masked: use_mask != 0
 * and gq < min_gq) and every allele index the mode reads lies in [0, A).  n_out[v] receives the number of usable cells.  Record v
 * owns the slots [var_allele_off[v], var_allele_off[v + 1]) of het_out and of hom_out, one per allele, REF first: a usable diploid
 * cell with gt1 == gt2 adds 1 to hom[slot gt1]; one with gt1 != gt2 adds 1 to het[slot gt1] and 1 to het[slot gt2]; a usable
 * haploid cell adds 1 to hom[slot gt1].  So per diploid record the sum over its slots of het + 2 * hom is 2 * n_out[v].  This is
 * NOT mg_site_counts' rule, which counts the valid index of a cell whose other index is invalid: here such a cell counts nowhere
 * (the genotyper makes no such cells).  accumulate != 0 adds to what the three arrays hold (the groups of a cohort larger than
 * 64 are summed this way); accumulate == 0 overwrites every slot of every record and every n_out.  Nothing is written outside a
 * record's slots.  n_vars == 0 is legal.  n_planes out of range, a NULL gt1 / var_allele_off / n_out with n_vars > 0, a NULL gt2 in
 * diploid mode, a NULL gq under the mask, a NULL het_out or hom_out with slots: MG_ERR_ARG.  The host form synchronises; the
 * device form (every array a device pointer) is asynchronous on the context's stream.
 * mg_hwe_exact: item i is one (record, ALT): n[i] usable diploid cells, het[i] of them with exactly one copy of the allele,
 * hom[i] with two.  hwe_out[i] is the two-sided exact P value (the sum of the probabilities, given the allele count, of all
 * heterozygote counts no likelier than the observed one), exc_het_out[i] the one-sided one for an excess of heterozygotes (the
 * counts at and above the observed one).  Both are pure functions of (n, het, hom).  In 64-bit unsigned integers, `/` the integer
 * division:  na = het + 2 * hom, nb = 2 * n - na, r = min(na, nb);  mid = r * (2 * n - r) / (2 * n), 0 when n == 0, raised by one
 * if its parity differs from r's;  hr = (r - mid) / 2, hc = n - mid - hr.  Unnormalised terms in IEEE doubles:  q(mid) = 1.0;
 * downward, while h > 1:  q(h - 2) = q(h) * ( double(h * (h - 1)) / double(4 * (hr + 1) * (hc + 1)) ), then hr++, hc++;  upward,
 * restarting from mid, while h <= r - 2:  q(h + 2) = q(h) * ( double(4 * hr * hc) / double((h + 2) * (h + 1)) ), then hr--, hc--.
 * Every ratio is formed first and then multiplied.  q_obs = q(het).  Three sums are added in visiting order (mid, downward,
 * upward): S all terms, L the terms with q <= q_obs, G the terms with h >= het;  hwe = min(L / S, 1.0), exc_het = min(G / S, 1.0).
 * Every step is one correctly rounded operation, so the results are the same bits on every device and in every restatement
 * that keeps the order.  n == 0 gives 1.0 and 1.0.  An item with het + hom > n, or with n > MG_HWE_MAX_N (a bound on one thread's
 * walk, 2^23 steps, far below where the 64-bit products above would wrap), gets a quiet NaN in both outputs.  n_items == 0 is legal; a
 * NULL array with n_items > 0: MG_ERR_ARG.  One thread walks one item, r / 2 steps.  The host form synchronises; the device form
 * is asynchronous on the context's stream.
 * mg_hwe_stats (waits): ms_out[2], device milliseconds of the most recent mg_site_geno_counts* and of the most recent
 * mg_hwe_exact*; 0 for a kind not called yet, MG_ERR_STATE when neither was.
 * The calls keep their device copies of their tables and their events apart from the encoders', the site tags', the pair
 * table's and the sample table's: a call of one kind between two of another changes nothing in either. */
#define MG_HWE_MAX_N (1u << 24)
int mg_site_geno_counts(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                        int32_t min_gq, const uint32_t *var_allele_off, int accumulate, uint32_t *n_out, uint32_t *het_out, uint32_t *hom_out);
int mg_site_geno_counts_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                               int32_t min_gq, const void *d_var_allele_off, int accumulate, void *d_n_out, void *d_het_out, void *d_hom_out);
int mg_hwe_exact(mg_ctx *ctx, size_t n_items, const uint32_t *n, const uint32_t *het, const uint32_t *hom, double *hwe_out, double *exc_het_out);
int mg_hwe_exact_device(mg_ctx *ctx, size_t n_items, const void *d_n, const void *d_het, const void *d_hom, void *d_hwe_out, void *d_exc_het_out);
int mg_hwe_stats(mg_ctx *ctx, float *ms_out);

/* ---- the LD table of a multi-sample call set ----------------------------------------
 * Record against record along the samples: for a record and each of the `window` records behind it, the squared correlation r2 of
 * the two dosages over the samples that contribute in both.  There is no reference call to cite: the reference genotypes one
 * individual per run and has nothing that looks across samples.
 * mg_pack_site_dosage: inputs and the CALLED rule exactly as for mg_pack_dosage: gt1 / gt2 / gq [n_planes][n_vars] int32,
 * plane-major, n_planes 1..64; gt2 is not read in haploid mode and may be NULL, gq not unless use_mask; a cell is called unless
 * use_mask != 0 and its gq < min_gq; var_allele_off ([n_vars + 1]) is required.  A cell (p, v) CONTRIBUTES when record v has two
 * alleles, the cell is called and every allele index the mode reads is 0 or 1; its dosage is gt1 + gt2 (haploid: 2 * gt1).
 * sites_out is uint64_t [3][n_vars] -- the transpose of mg_pack_dosage's layout, bits over samples per record: bit p of
 * sites_out[d * n_vars + v] is set exactly when the cell (p, v) contributes with dosage d.  Bits at and above n_planes are 0.
 * Every word is written, the caller need not clear it; n_vars == 0 is legal and writes nothing.  Argument errors as
 * mg_pack_dosage's: n_planes out of range, a NULL var_allele_off, a NULL gt1 or sites_out with n_vars > 0, a NULL gt2 in diploid
 * mode, a NULL gq under the mask: MG_ERR_ARG.
 * mg_ld_window: sites is uint64_t [n_groups][3][n_vars], the groups' mg_pack_site_dosage outputs over the same records
 * (n_groups 1..MG_LD_MAX_GROUPS: 16,384 samples, the cohort's own limit); chrom and pos are uint32_t [n_vars]; window is
 * 1..MG_LD_MAX_WINDOW; min_r2 is finite and in [0, 1]; min_n is at least 1; n_first <= n_vars -- each of these else MG_ERR_ARG, as a
 * NULL sites / chrom / pos with n_vars > 0, a NULL row_off_out or n_pairs_out, a NULL pairs_out with pairs_cap > 0.
 * The pair (i, j) is ELIGIBLE when i < n_first, i < j <= i + window, j < n_vars, chrom[i] == chrom[j], and max_bp == 0 or
 * |pos[j] - pos[i]| <= max_bp (the difference formed in signed 64-bit).  Records at and beyond n_first serve as partners only:
 * a caller walks a long table in chunks with a look-ahead of `window` records, and every pair comes out exactly once.
 * Over all groups and the samples whose cells contribute in BOTH records, with dosages x at i and y at j:  n the number of such
 * samples, Sx, Sy, Sxx, Syy, Sxy the sums of x, y, x x, y y, x y -- popcounts of ANDs of the six words and their ORs, the groups'
 * words only ever ANDed within a group and the popcounts summed, so the result does not depend on how a cohort is cut into groups.
 * In signed 64-bit:  cov = n Sxy - Sx Sy,  vx = n Sxx - Sx Sx,  vy = n Syy - Sy Sy.  With n <= 2^14 each of the three is at most
 * 2^30 in magnitude, so cov cov and vx vy are at most 2^60 and nothing wraps.  The pair is DEFINED when n >= min_n, vx > 0 and
 * vy > 0; then r2 = double(uint64(cov cov)) / double(uint64(vx vy)): each conversion rounds once, to nearest even, and there is
 * one division, so every step is one correctly rounded operation and the bits are the same on every device and in every
 * restatement.  The pair is EMITTED when it is eligible, defined and r2 >= min_r2.
 * An emitted pair is one mg_ld_pair: i, j, n, sign (+1, -1 or 0: the sign of cov) and r2.  Emitted pairs are ordered by i, then j
 * ascending, whatever the launch geometry; row_off_out is uint64_t [n_first + 1], record i's pairs are
 * pairs_out[row_off_out[i] .. row_off_out[i + 1]).  The buffer contract is mg_format_calls': *n_pairs_out (a HOST pointer in both
 * forms) always receives the number of pairs needed; when that exceeds pairs_cap the call returns MG_ERR_LIMIT, nothing is written
 * at or behind pairs_cap, row_off_out is valid all the same, and the caller may come again with a larger buffer.  n_first == 0 and
 * n_vars == 0 are legal: row_off_out[0] = 0.
 * Each call has a host form, which synchronises, and a _device form (every array a device pointer), asynchronous on the context's
 * stream -- mg_ld_window_device until it reads the total back, behind its write pass.
 * mg_ld_stats (waits): ms_out[2], device milliseconds of the most recent mg_pack_site_dosage* and of the most recent mg_ld_window*
 * (its three passes together); 0 for a kind not called yet, MG_ERR_STATE when neither was.
 * The calls keep their device copies of their tables and their events apart from every other section's: a call of another kind
 * in between changes nothing. */
#define MG_LD_MAX_GROUPS 256
#define MG_LD_MAX_WINDOW 1024
typedef struct mg_ld_pair {
    uint32_t i, j, n;
    int32_t sign;
    double r2;
} mg_ld_pair; /* 24 bytes */
int mg_pack_site_dosage(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const int32_t *gt1, const int32_t *gt2, const int32_t *gq, int use_mask,
                        int32_t min_gq, const uint32_t *var_allele_off, uint64_t *sites_out);
int mg_pack_site_dosage_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, int haploid, const void *d_gt1, const void *d_gt2, const void *d_gq, int use_mask,
                               int32_t min_gq, const void *d_var_allele_off, void *d_sites_out);
int mg_ld_window(mg_ctx *ctx, size_t n_vars, size_t n_first, uint32_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, uint32_t window,
                 uint64_t max_bp, uint32_t min_n, double min_r2, mg_ld_pair *pairs_out, size_t pairs_cap, uint64_t *row_off_out, uint64_t *n_pairs_out);
int mg_ld_window_device(mg_ctx *ctx, size_t n_vars, size_t n_first, uint32_t n_groups, const void *d_sites, const void *d_chrom, const void *d_pos, uint32_t window,
                        uint64_t max_bp, uint32_t min_n, double min_r2, void *d_pairs_out, size_t pairs_cap, void *d_row_off_out, uint64_t *n_pairs_out);
int mg_ld_stats(mg_ctx *ctx, float *ms_out);

/* ---- IBS0-free segments per pair of samples ------------------------------------------
 * Where along the records two samples share genotypes.  There is no reference call to cite: the reference genotypes one individual
 * per run.  The cells CONTRIBUTE, with dosage 0, 1 or 2, exactly as for mg_pack_dosage / mg_pack_site_dosage.
 * mg_sites_to_planes: sites is uint64_t [n_groups][3][n_vars], the groups' mg_pack_site_dosage outputs over the same records, as
 * mg_ld_window takes them (n_groups 1..MG_LD_MAX_GROUPS).  planes_out is uint64_t [64 * n_groups][3][W], W = ceil(n_vars / 64), laid
 * out as mg_pack_dosage's: bit v & 63 of word v >> 6 of plane 64 g + p, dosage d, equals bit p of sites[g][d][v] -- the same cells in
 * the records' order of `sites`, whatever the batches were.  Every word is written, the bits at and beyond n_vars are 0; n_vars == 0
 * is legal and writes nothing.  A NULL sites or planes_out with n_vars > 0, n_groups out of range: MG_ERR_ARG.
 * The segments.  For a pair of samples a < b (indexes over all groups, sample 64 g + p is bit p of group g) every record is DISC (both
 * cells contribute, dosages {0, 2}), CONC (both contribute, not DISC; IBS2 when the dosages are equal) or NEUT.  The pair's state is open
 * or closed, chrom, start_pos, end_pos, n, ibs2.  At record v, in this order: an open state whose chrom differs from chrom[v] closes; DISC
 * closes an open state; CONC opens a closed state (chrom[v], start_pos = pos[v], n = ibs2 = 0), then end_pos = pos[v], n += 1, ibs2 += 1
 * when IBS2; NEUT does nothing.  Closing emits the segment when n >= min_records and end_pos - start_pos >= min_bp (the difference
 * formed in signed 64-bit).
 * mg_ibd_begin: n_samples is 2..MG_IBD_MAX_SAMPLES, min_records at least 1, min_bp at most 2^63 - 1, else MG_ERR_ARG.  It allocates the
 * device-resident state of all n (n - 1) / 2 pairs, five uint32_t per pair (2.7 GB at the limit), all closed; MG_ERR_NOMEM when that does
 * not fit.  A second begin discards the first.  mg_ibd_end frees the state (and is legal without one).
 * mg_ibd_step walks the next n_vars records: sites as above with n_groups == ceil(n_samples / 64) (else MG_ERR_ARG), chrom and pos
 * uint32_t [n_vars]; a NULL among them with n_vars > 0, a NULL n_segs_out, a NULL segs_out with segs_cap > 0: MG_ERR_ARG.  Without a begin:
 * MG_ERR_STATE.  Record 0's chrom is compared with the last record of the step before.  flush != 0 closes every open state behind the
 * last record; n_vars == 0 is legal with and without it.  The segments closed in this step come out ordered by a, then b, then along the
 * records.  *n_segs_out (a HOST pointer in both forms) always receives the number needed; when that exceeds segs_cap the call returns
 * MG_ERR_LIMIT, writes nothing to segs_out and does NOT advance the state: the same call with a larger buffer is correct.
 * Working memory of a step, from the context: the planes of its records (24 n_groups bytes per record) and 12 bytes per pair for
 * the segment counts and their offsets.
 * The host forms synchronise.  The device forms take device pointers; mg_sites_to_planes_device is asynchronous on the context's stream,
 * mg_ibd_step_device waits for the total between its length pass and its write pass.
 * mg_ibd_stats (waits): ms_out[2], device milliseconds of the most recent transpose (a step's own included) and of the most recent step
 * (everything it put on the stream); 0 for a kind not called yet, MG_ERR_STATE when neither was. */
#define MG_IBD_MAX_SAMPLES 16384
typedef struct mg_ibd_seg {
    uint32_t a, b, chrom, start_pos, end_pos, n, ibs2, zero;
} mg_ibd_seg; /* 32 bytes */
int mg_sites_to_planes(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const uint64_t *sites, uint64_t *planes_out);
int mg_sites_to_planes_device(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const void *d_sites, void *d_planes_out);
int mg_ibd_begin(mg_ctx *ctx, uint32_t n_samples, uint32_t min_records, uint64_t min_bp);
int mg_ibd_step(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const uint64_t *sites, const uint32_t *chrom, const uint32_t *pos, int flush, mg_ibd_seg *segs_out,
                size_t segs_cap, uint64_t *n_segs_out);
int mg_ibd_step_device(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const void *d_sites, const void *d_chrom, const void *d_pos, int flush, void *d_segs_out,
                       size_t segs_cap, uint64_t *n_segs_out);
int mg_ibd_end(mg_ctx *ctx);
int mg_ibd_stats(mg_ctx *ctx, float *ms_out);

/* ---- the genetic relationship matrix (GRM) ---------------------------------------------
 * For every pair of samples, the sum over the records of the product of their standardised dosages, in fixed point and exact.  There is no
 * reference call to cite: the reference genotypes one individual per run.  The cells CONTRIBUTE, with dosage 0, 1 or 2, exactly as for
 * mg_pack_dosage / mg_pack_site_dosage.  sites is uint64_t [n_groups][3][n_vars], the groups' mg_pack_site_dosage outputs side by side as
 * mg_ibd_step takes them: sample 64 g + p is bit p of group g, n_groups == ceil(n_samples / 64) (else MG_ERR_ARG); the bits at and beyond
 * n_samples are masked off by the library.
 * Per record, over the whole cohort, n_d = the set bits of dosage d.  Diploid: n = n0 + n1 + n2, AN = 2 n, AC = n1 + 2 n2, D = 2 AC (AN - AC).
 * Haploid (the pack gives dosages 0 and 2; dosage-1 bits are ignored): n = n0 + n2, AN = n, AC = n2, D = 4 AC (AN - AC).  D < 2^31.
 *   q_d = rint((d AN - 2 AC) 1024 / sqrt((double)D)),  d = 0, 1, 2:  IEEE binary64 sqrt, one divide, round-half-even
 * -- the standardised dosage (d - 2p) / sqrt(2p (1 - p)), or its haploid counterpart, with MG_GRM_SHIFT fraction bits.  The record ENTERS when
 * D > 0, n >= min_n, min(AC, AN - AC) 1000000 >= maf_ppm AN (64-bit integers) and every |q_d| <= MG_GRM_MAX_Q (both balanced base-256 digits of
 * q fit a signed byte; a minor allele frequency of about 0.002 and up).
 * For samples a <= b (a == b included), over the entering records where both cells contribute: N_ab their number, S_ab the signed 64-bit sum
 * of q_{x_a} q_{x_b}.  The GRM value is S_ab / (2^20 N_ab).  Integer sums: the same values whatever the steps, pieces and order of summation.
 * mg_grm_weights: q_out is int16_t [n_vars][4] -- q0 q1 q2 1 for a record that enters, 0 0 0 0 for one that does not.  n_samples is
 * 1..MG_GRM_MAX_SAMPLES, maf_ppm 0..500000, min_n at least 1, else MG_ERR_ARG; n_vars == 0 is legal.
 * mg_grm_begin: the same ranges.  It allocates the device-resident state of all n (n + 1) / 2 pairs, 16 bytes per pair (2.1 GB at the
 * limit), all zero; MG_ERR_NOMEM when that does not fit.  A second begin discards the first.  mg_grm_end frees the state (and is legal
 * without one).
 * mg_grm_step adds the next n_vars records (n_vars == 0 is legal).  Without a begin: MG_ERR_STATE.  Working memory of a step, from the
 * context: 3 bytes per record and sample (samples padded to 32, records to 64) plus 8 bytes per record, for a piece of the step at a time;
 * the pieces are cut so that the 3-byte part stays at or under 384 MiB (option grm_scratch_mb), or one 64-record slice where that is more.
 * mg_grm_read (waits; callable between steps): sum_out int64_t and n_out uint64_t [n (n + 1) / 2], pair (a, b), a <= b, row-major --
 * at a (2 n - a + 1) / 2 + b - a; records_out[0] the records seen since the begin, [1] those that entered.  Host pointers.
 * The host forms synchronise.  The device forms take device pointers and are asynchronous on the context's stream.
 * mg_grm_stats (waits): ms_out[3], device milliseconds of the most recent step -- [0] weights and expansion, [1] the Gram kernel, over all
 * its pieces -- and [2] of the most recent read; 0 for a kind not called yet, MG_ERR_STATE when neither was. */
#define MG_GRM_MAX_SAMPLES 16384
#define MG_GRM_SHIFT 10
#define MG_GRM_MAX_Q 32639
int mg_grm_weights(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, uint32_t n_samples, const uint64_t *sites, int haploid, uint32_t maf_ppm, uint32_t min_n,
                   int16_t *q_out);
int mg_grm_weights_device(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, uint32_t n_samples, const void *d_sites, int haploid, uint32_t maf_ppm, uint32_t min_n,
                          void *d_q_out);
int mg_grm_begin(mg_ctx *ctx, uint32_t n_samples, int haploid, uint32_t maf_ppm, uint32_t min_n);
int mg_grm_step(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const uint64_t *sites);
int mg_grm_step_device(mg_ctx *ctx, size_t n_vars, uint32_t n_groups, const void *d_sites);
int mg_grm_read(mg_ctx *ctx, int64_t *sum_out, uint64_t *n_out, uint64_t *records_out);
int mg_grm_end(mg_ctx *ctx);
int mg_grm_stats(mg_ctx *ctx, float *ms_out);

/* ---- principal components: the leading eigenpairs of a symmetric matrix ---------------------
 * What GCTA and PLINK --pca make of a GRM, solved on the device.  There is no reference call to cite: the reference genotypes one
 * individual per run.  G is a real symmetric n x n matrix, resident in double.  The result is K eigenpairs (theta_i, v_i), i = 0 .. K - 1.
 *   Order.  The K ALGEBRAICALLY LARGEST eigenvalues, descending.
 *   Vectors.  Orthonormal.  Each vector's sign is fixed so that its component of largest magnitude is positive; among equal magnitudes
 *   the lowest index decides.
 *   Residual.  Per pair r_i = ||G v_i - theta_i v_i||_2 / s, s the largest |theta| of the final Rayleigh-Ritz block (all m values, not
 *   only the K returned), or 1 when that is 0.  s is written out.
 *   Convergence.  A pair is converged when r_i <= tol.  The solve stops when the first K pairs are converged, or at max_iters products;
 *   it always returns K pairs, and an unconverged result is MG_OK.
 *   Determinism.  No floating-point atomics and no reduction whose order depends on scheduling: every split of an n-long sum over waves
 *   and workgroups is a function of n alone (csrc/pca_plan.h).  Two solves of one matrix give the same bytes; the host form and the device
 *   form give the same bytes.
 *   Method.  Blocked subspace iteration with Rayleigh-Ritz on a block of m = min(n, roundup16(max(2 K, K + 16))) columns.  The start
 *   vectors are a counter hash of (row, column) (pca_hash_value; no library generator).  A step forms Y = G Q (one PRODUCT) and
 *   orthonormalises Y on the device by Cholesky QR, twice; a column whose pivot collapses is replaced by a fresh hashed vector and made
 *   orthogonal to the rest by the second pass, so the block keeps its full width on a matrix of any rank.  After every 4th product, and
 *   after the last one allowed: H = Q^T Y, its m x m eigenproblem (on the host, cyclic Jacobi in double; values algebraically
 *   descending), Q <- Q S, Y <- Y S, and the residual test on the columns of Y - Q diag(theta).  m == n: nothing to iterate, G itself goes
 *   through the small solver and 0 products are reported.
 *   Limit of the method.  It iterates by magnitude: a matrix with more than m - K eigenvalues below -theta_{K-1} cannot converge for pair
 *   K - 1; that is reported as not converged, not refused.  One large negative eigenvalue takes a block slot and is not among the K.
 * mg_pca_load_tri_f32: GCTA's .grm.bin layout -- the lower triangle row by row, diagonal included, n (n + 1) / 2 floats, element (i, j),
 * j <= i, at i (i + 1) / 2 + j -- expanded on the device to the resident symmetric matrix (8 n'^2 bytes, n' = n rounded up to 16: 2.1 GB at
 * the limit).  mg_pca_load_f64: row-major n x n doubles, of which only a[i][j], j <= i, is read and mirrored: the resident matrix is
 * symmetric by construction.  A second load discards the first; a matrix (or, in a host form, its input) that does not fit: MG_ERR_NOMEM.
 * n outside 1..MG_PCA_MAX_N or a NULL pointer: MG_ERR_ARG.  A value that is not finite is found by a device reduction over the load: the
 * host forms return MG_ERR_ARG with a message and keep no matrix; the _device forms take device pointers and are asynchronous on the
 * context's stream, so there the first mg_pca_solve* after the load returns it (and the matrix is gone).
 * mg_pca_solve: k is 1..min(n, MG_PCA_MAX_K), tol finite and > 0, max_iters >= 1, no pointer NULL, else MG_ERR_ARG; without a load
 * MG_ERR_STATE.  values_out[k], descending; vectors_out[k][n], one row per component; resid_out[k] = r_i; scale_out[1] = s; info_out[3]:
 * [0] the products G Q performed, [1] how many of the k pairs are converged, [2] m.  Callable repeatedly on one load: the matrix is not
 * modified.  Nothing outside these arrays is written.  mg_pca_solve_device takes the five outputs as device pointers; both forms wait
 * (a Rayleigh-Ritz step needs the host) and return with the result complete.
 * mg_pca_end frees the matrix (legal without a load).  mg_pca_stats (waits): ms_out[4], device milliseconds of the most recent solve --
 * [0] products, [1] orthonormalisation, [2] Rayleigh-Ritz (projection, block update, residual norms, and the device's wait for the
 * host's small solver), [3] total; MG_ERR_STATE before any solve. */
#define MG_PCA_MAX_N 16384
#define MG_PCA_MAX_K 32
int mg_pca_load_tri_f32(mg_ctx *ctx, uint32_t n, const float *tri);
int mg_pca_load_f64(mg_ctx *ctx, uint32_t n, const double *full);
int mg_pca_load_tri_f32_device(mg_ctx *ctx, uint32_t n, const void *d_tri);
int mg_pca_load_f64_device(mg_ctx *ctx, uint32_t n, const void *d_full);
int mg_pca_solve(mg_ctx *ctx, uint32_t k, double tol, uint32_t max_iters, double *values_out, double *vectors_out, double *resid_out, double *scale_out,
                 uint32_t *info_out);
int mg_pca_solve_device(mg_ctx *ctx, uint32_t k, double tol, uint32_t max_iters, void *d_values_out, void *d_vectors_out, void *d_resid_out, void *d_scale_out,
                        void *d_info_out);
int mg_pca_end(mg_ctx *ctx);
int mg_pca_stats(mg_ctx *ctx, float *ms_out);

/* ---- allele priors re-estimated from the cohort -------------------------------------
 * mg_genotype_cohort: the batch's allele frequencies are re-estimated from all of its planes (a few EM steps from the panel's
 * priors, anchored to them), then every cell is genotyped under the result.  The reference genotypes one individual and has no
 * such step: there is NO reference call to cite for the estimate.  The per-cell part is mg_genotype's -- VB::genotype
 * (var_block.hpp:224-330) and the normalise / first-strict-max / GQ step (:366-394).
 * Inputs as for mg_genotype, plus planes: cov is [n_planes][slots] uint32, plane-major, slots = var_allele_off[n_vars]; freq is
 * [slots] float, the panel's priors f0; error_rate, max_cov, haploid; iters T (0..64); weight w (finite, >= 0).  n_planes 1..64.
 * For a record with A alleles, ploidy = 1 in haploid mode, else 2.
 *   Status.  The status of a plane's cell is the one mg_genotype gives it (MG_GT_*); it depends on the coverages alone.
 *   Which records.  A record is re-estimated when 2 <= A <= MG_PRIOR_MAX_ALLELES and T > 0.  Any other record keeps f = f0,
 *   reports n_informative = 0 and is genotyped exactly as mg_genotype genotypes it.
 *   Iteration t = 1..T starts from f = f_{t-1}, f_0 = f0.
 *     Posteriors.  For every plane p whose status is MG_GT_NORMAL: the raw values of all genotypes in the reference's list order
 *     (a outer, c >= a inner; haploid: the alleles) under f, and their sum 0.0 + v0 + v1 + .., left to right, exactly as
 *     mg_genotype makes them.  Plane p COUNTS in this iteration when that sum is finite and > 0; its posteriors are q_g = v_g / sum.
 *     Expected copies.  For each allele a, e_p[a] starts at 0.0 and walks the genotype list in order: + 2.0 * q_g for the
 *     homozygous genotype of a, + q_g for every heterozygous genotype that contains a; in haploid mode + q_g for genotype a.  A
 *     plane that does not count has e_p[a] = +0.0.
 *     Sum over planes, in a fixed tree order.  P' is the smallest power of two >= n_planes; x[i] = e_i[a] for i < n_planes and
 *     +0.0 above; for s = P'/2, P'/4, .., 1: x[i] = x[i] + x[i + s] for i < s; c[a] = x[0].  n is the number of planes that count.
 *     Update.  n == 0: the frequencies stay as they are.  Otherwise for every ALT allele a >= 1:
 *       f_t[a] = (float)((c[a] + w * (double)f0[a]) / ((double)(ploidy * n) + w))
 *     -- the multiply, the add, the divide and the cast each rounded on its own -- and the REF allele follows the panel
 *     parser's rule: acc = 0.0 (double), plus 0.f, plus the ALT values f_t[1], f_t[2], .. in order; f_t[0] = (float)(1.0 - acc),
 *     or 0.0f when that is negative.
 *   w anchors the estimate to the panel's prior with the weight of w allele copies (a MAP estimate under a Dirichlet prior); it
 *   keeps a small cohort from driving a frequency to an absorbing 0.  A record whose f_t equals f_{t-1} bit for bit stops early:
 *   the following iterations would repeat it.
 * Outputs after T iterations: freq_out[slots] = f_T; n_informative[v] = n of the last iteration that ran; gt1 / gt2 / gq / status
 * [n_planes][n_vars], every plane's cell as mg_genotype makes it from (cov_p, f_T); probs (optional, with var_gt_off
 * [n_vars + 1]) [n_planes][var_gt_off[n_vars]], laid out as mg_cells takes it.
 * Numerics: nothing is contracted into an FMA; every logf and exp is mg_genotype's restatement of the host libm's, every ln(n)
 * for n < 65536 its host-made table, so with every record's total coverage below 65536 the whole result is bit-identical to a
 * CPU restatement of the above.  At or beyond that total: the cells of a record the entry does not re-estimate are computed
 * again on the host with libm by the host form (as in mg_genotype) and are bit-identical at every total; a re-estimated record
 * uses the device's log(double) there, in both forms, as mg_genotype_device does -- with at most 8 alleles that takes a
 * max_cov of 8192 or more.
 * n_vars == 0 is legal.  iters > 64, a negative or non-finite weight, n_planes out of range, a NULL required array with
 * n_vars > 0, probs without var_gt_off: MG_ERR_ARG, nothing written.  The context need not be in cohort mode: the call reads
 * arrays and no counters.  The host form synchronises; the device form (every array a device pointer) is asynchronous on the
 * context's stream.  mg_cohort_prior_stats (waits): ms_out[1], device milliseconds of the most recent mg_genotype_cohort*;
 * MG_ERR_STATE before the first. */
#define MG_PRIOR_MAX_ALLELES 8
int mg_genotype_cohort(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off,
                       float error_rate, int max_cov, int haploid, uint32_t iters, double weight, float *freq_out, uint32_t *n_informative,
                       int32_t *gt1, int32_t *gt2, int32_t *gq, uint8_t *status, double *probs, const uint64_t *var_gt_off);
int mg_genotype_cohort_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_freq, const void *d_var_allele_off,
                              float error_rate, int max_cov, int haploid, uint32_t iters, double weight, void *d_freq_out, void *d_n_informative,
                              void *d_gt1, void *d_gt2, void *d_gq, void *d_status, void *d_probs, const void *d_var_gt_off);
int mg_cohort_prior_stats(mg_ctx *ctx, float *ms_out);

/* mg_estimate_priors: the estimate of mg_genotype_cohort alone, for 1..MG_PRIOR_WIDE_MAX_PLANES planes; it makes no calls.
 * Everything in the definition above stays as it is -- which records are re-estimated, status, posteriors, the expected copies
 * per plane, the update with its separately rounded operations, the REF rule, n == 0, the early stop, n_informative = n of the
 * last iteration that ran.  Only the sum over planes is extended:
 *   Planes are taken in the order given and cut into chunks of 64: chunk j holds planes 64j .. min(64j + 64, P) - 1.
 *   C_j[a] is the fixed tree above over the chunk's planes, padded with +0.0 to the smallest power of two >= the chunk's plane
 *   count.  c[a] = C_0[a], then c[a] = c[a] + C_j[a] for j = 1, 2, .. in order, each add rounded on its own.  n is the integer
 *   count of the planes that count over all chunks.
 * For P <= 64 this is mg_genotype_cohort's sum, bit for bit.  Every e_p[a] is >= +0.0 and x + (+0.0) = x for such x, so padding
 * a short chunk to 64 lanes gives the same C_j as padding it to its own power of two: the kernel runs every chunk at segment
 * width 64 when P > 64.  The order is fixed so that the result is reproducible and does not depend on how a caller groups its
 * planes; chunks are cut on the plane index alone.
 * Outputs: freq_out[slots] = f_T; n_informative[n_vars].  A record that is not re-estimated (A < 2, A > MG_PRIOR_MAX_ALLELES,
 * T = 0) gets freq_out = f0 and n_informative = 0.  Nothing outside freq_out[0 .. slots) and n_informative[0 .. n_vars) is
 * written.  The cells are genotyped afterwards, per group of <= 64 planes, by mg_genotype_cohort(iters = 0, freq = f_T), which
 * genotypes each cell exactly as mg_genotype does from (cov_p, f_T) -- what mg_genotype_cohort(iters = T)'s last step does.  One
 * limit: with iters = 0 the host form of mg_genotype_cohort recomputes the cells of a record at or above a total coverage of
 * 65536 with libm, where mg_genotype_cohort(iters = T) keeps the device's log(double) for a re-estimated record; the two-step
 * result equals the one-step result bit for bit for totals < 65536 (leaving that range takes a max_cov of 8192 or more).
 * Numerics are mg_genotype_cohort's: no FMA contraction, its logf and exp, the host-made ln(n) table; with every record's total
 * coverage below 65536 the result is bit-identical to a CPU restatement, beyond that it uses the device's log(double).
 * MG_PRIOR_WIDE_MAX_PLANES is a design choice (256 chunks), not a limit of the method.
 * n_vars == 0 is legal.  iters > 64, a negative or non-finite weight, n_planes 0 or above MG_PRIOR_WIDE_MAX_PLANES, a NULL
 * required array with n_vars > 0: MG_ERR_ARG, nothing written.  The host form synchronises; the device form (every array a
 * device pointer) is asynchronous on the context's stream.  mg_estimate_priors_stats (waits): ms_out[1], device milliseconds of
 * the most recent mg_estimate_priors* (an event pair of its own); MG_ERR_STATE before the first. */
#define MG_PRIOR_WIDE_MAX_PLANES 16384
int mg_estimate_priors(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const float *freq, const uint32_t *var_allele_off,
                       float error_rate, int max_cov, int haploid, uint32_t iters, double weight, float *freq_out, uint32_t *n_informative);
int mg_estimate_priors_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_freq, const void *d_var_allele_off,
                              float error_rate, int max_cov, int haploid, uint32_t iters, double weight, void *d_freq_out, void *d_n_informative);
int mg_estimate_priors_stats(mg_ctx *ctx, float *ms_out);

/* ---- the sample columns of a multi-sample BCF --------------------------------------
 * mg_format_calls' rows in BCF2's binary form (VCF/BCF specification v4.3, section 6.3.3; restated from the published layout,
 * parity with htslib unpinned).  The cells (mg_cells, with its field rules), the host and _device forms, the stream behaviour and
 * the buffer contract are mg_format_calls': *bytes_out (a HOST pointer in both forms) always receives the bytes needed,
 * MG_ERR_LIMIT when that exceeds out_cap, nothing written at or behind out_cap, the out_cap bytes in front of it the output's
 * first, row_off_out valid all the same, n_vars == 0 legal.  Row v = out[row_off_out[v] .. row_off_out[v + 1]) is exactly the
 * record's per-sample ("indiv") block, its length the record's l_indiv: two fields, and one more each with cov, MG_CELLS_GP and
 * MG_CELLS_PL, in this order --
 *   GT    typed_int(keys->gt),  desc(ploidy, T), for every plane `ploidy` values (1 in haploid mode, else 2): allele index a
 *         as (a + 1) << 1, unphased; a cell with use_mask != 0 and gq < min_gq writes 0 (missing) for each of its values
 *   GQ    typed_int(keys->gq),  desc(1, T), one value per plane, as it is, mask or no mask
 *   COVS  typed_int(keys->cov), desc(A, T), for every plane the record's A = var_allele_off[v + 1] - var_allele_off[v] values
 *         (int32_t)cov[..]
 *   GP    typed_int(keys->gp),  desc(G, 5), for every plane the record's G float32
 *   PL    typed_int(keys->pl),  desc(G, T), for every plane the record's G values of type T
 * desc(n, t): the byte n << 4 | t for n < 15, else 0xF0 | t and typed_int(n).  typed_int(x): desc(1, t) and x in the smallest of
 * int8 (t = 1), int16 (2), int32 (3) that holds it.  Little endian.  T of a field of a record is the smallest type holding every
 * value of the field over all planes with BCF's reserved codes kept free: int8 for [-120, 127], int16 for [-32760, 32767], else
 * int32 (a field without values: int8).  An int32 value inside int32's reserved range [INT32_MIN, INT32_MIN + 7] is written as
 * it is: what a reader makes of it is the caller's business.
 * GP: a printable value is stored as (float)p, IEEE round to nearest even, float denormals kept (1e-40 does not become 0; the
 * conversion is done in integers); an unprintable one as the missing float 0x7F800001; a cell that is not MG_GT_NORMAL as
 * 0x7F800001 followed by G - 1 end-of-vector floats 0x7F800002, which is what `.` for a vector is in BCF.
 * PL: T is the smallest type that holds every value of the field over all planes that is not MG_PL_MISSING, by the rule above (a
 * field without such a value: int8).  MG_PL_MISSING is written as T's missing code -- 0x80, 0x8000, 0x80000000, in int32 the
 * sentinel itself --, a cell whose values are all missing as that code followed by G - 1 end-of-vector codes (0x81, 0x8001,
 * 0x80000001).
 * Where this departs from the text: an allele index outside [0, 2^30 - 2] has no code and writes 0 (missing), where
 * mg_format_calls prints the index as it is.  mg_bcf_keys holds the header's dictionary indexes, >= 0; cov, gp and pl are not read
 * without cov, MG_CELLS_GP and MG_CELLS_PL.  A NULL cells or keys pointer: MG_ERR_ARG.
 * mg_bcf_stats (waits): ms_out[3], device milliseconds of the most recent call's length pass, scan and write pass;
 * MG_ERR_STATE before the first call. */
typedef struct mg_bcf_keys {
    int32_t gt, gq, cov, gp, pl;
} mg_bcf_keys;
int mg_encode_calls_bcf(mg_ctx *ctx, const mg_cells *cells, const mg_bcf_keys *keys, uint8_t *out, size_t out_cap, uint64_t *row_off_out, uint64_t *bytes_out);
int mg_encode_calls_bcf_device(mg_ctx *ctx, const mg_cells *cells, const mg_bcf_keys *keys, void *d_out, size_t out_cap, void *d_row_off_out,
                               uint64_t *bytes_out);
int mg_bcf_stats(mg_ctx *ctx, float *ms_out);

/* ---- Phred-scaled genotype likelihoods (PL), prior-free -----------------------------
 * The likelihood part of the genotyper alone: what mg_genotype computes as log_post and multiplies with the allele-frequency prior
 * before anything leaves it.  No frequencies are read and no cohort mode is needed.  cov is [n_planes][var_allele_off[n_vars]],
 * plane-major, as mg_genotype_cohort takes it; pl_out is [n_planes][var_gt_off[n_vars]]; n_planes is 1..64, cap >= 1; n_vars == 0 is
 * legal.  A bad argument returns MG_ERR_ARG and writes nothing.
 * The values of a record are in VCF order: genotype j/k (j <= k) at index k (k + 1) / 2 + j of the record's slice, in haploid mode
 * the allele (probs of the genotype calls is in the reference's order; the encoders copy under MG_CELLS_PL).
 * The cell (p, v), A the record's alleles, G = A (haploid) or A (A + 1) / 2:
 *   1. if any (int)cov[a] > max_cov, all G values are MG_PL_MISSING (the over-covered cell the reference refuses to genotype);
 *   2. if A == 1, the one value is 0 and nothing is computed;
 *   3. if A == 0, nothing is written;
 *   4. otherwise lp_g, for every genotype g, is the log_post of the genotyper with the same operations in the same order (the
 *      host-made ln table, log_binomial, every (float)count * constant product rounded to float before it joins the double sum,
 *      the error term of a heterozygote only for A > 2, no FMA contraction); a cell of total coverage 0 comes out as all zeros,
 *      the honest likelihood of no data, and is not missing;
 *   5. M is the largest finite lp_g; if there is none, every value of the cell is missing;
 *   6. a NaN or +inf lp_g gives a missing value; otherwise d = M - lp_g, x = d * K with K = 0x1.15f2ced384f29p+2 (the double
 *      nearest to 10 / ln 10), PL = cap when x >= (double)cap, else (int32_t)(x + 0.5) -- so -inf gives cap; the subtract, the
 *      multiply and the add each rounded on their own.
 * With every record's total coverage below 65536 the result is bit-identical to a CPU restatement of this; at or above it ln(n) is
 * the device's log(double), as in mg_genotype_device, in both forms.  The host form checks that every record's slice of var_gt_off
 * is G long (MG_ERR_ARG); the device form cannot, and leaves such a record alone.  The _device form takes device pointers and is
 * asynchronous on the context's stream.  mg_pl_stats (waits): ms_out[1], device milliseconds of the most recent call;
 * MG_ERR_STATE before the first. */
int mg_phred_likelihoods(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const uint32_t *cov, const uint32_t *var_allele_off, const uint64_t *var_gt_off,
                         float error_rate, int max_cov, int haploid, int32_t cap, int32_t *pl_out);
int mg_phred_likelihoods_device(mg_ctx *ctx, size_t n_vars, uint32_t n_planes, const void *d_cov, const void *d_var_allele_off, const void *d_var_gt_off,
                                float error_rate, int max_cov, int haploid, int32_t cap, void *d_pl_out);
int mg_pl_stats(mg_ctx *ctx, float *ms_out);

/* ---- index payloads  (bloom_filter.hpp:127-146, kmap.hpp:52-82) ----------- */

/* BF: _mode, _size, bit words (ceil(size/64) u64), counters (n_set u16).
 * Call with NULL buffers to query sizes first. */
int mg_bf_export(mg_ctx *ctx, int which, uint64_t *words_out, uint16_t *counts_out);
int mg_bf_import(mg_ctx *ctx, int which, int mode, uint64_t size_bits, const uint64_t *words,
                 const uint16_t *counts, uint64_t n_counts);
/* The same payload in sparse form (what the index file holds): the n_set ascending
 * bit positions (= counter order) and the counters.  Export needs a finalised filter. */
int mg_bf_export_sparse(mg_ctx *ctx, int which, uint64_t *positions_out, uint16_t *counts_out);
int mg_bf_import_sparse(mg_ctx *ctx, int which, int mode, uint64_t size_bits, const uint64_t *positions,
                        const uint16_t *counts, uint64_t n);
/* KMAP: n keys as NUL-terminated rows of `stride` bytes + values.  stride >= k + 1, and beyond the longest key of another
 * length the map holds (MG_ERR_ARG otherwise: a key cut short would name another key); MG_MAX_KMER + 1 always fits */
int mg_map_export(mg_ctx *ctx, char *rows_out, size_t stride, int32_t *vals_out);
/* KMAP::add_key of every row, then the key of row i set to vals[i] (vals may be NULL: insert only).  A file may repeat a key
 * or name one that is already present: the last row that names a key gives its value, as when the reference reads row by row. */
int mg_map_import(mg_ctx *ctx, const char *rows, size_t stride, size_t n, const int32_t *vals);

/* ---- introspection for tests / profiling ---------------------------------- */

/* hash % size of BF::_get_hash for each row (bloom_filter.hpp:67-74,84) */
int mg_debug_bf_index(mg_ctx *ctx, int which, const char *rows, size_t stride, size_t n, uint64_t *idx_out);
/* same from packed k-mers of length klen (1..64), MSB-first right-aligned */
int mg_debug_packed_index(mg_ctx *ctx, int which, const uint64_t *hi, const uint64_t *lo, size_t n, uint32_t klen,
                          uint64_t *idx_out);
/* the exclusive scan mg_bf_finalize runs over its tile sums, on n values of the caller's: x is replaced by its exclusive prefix
 * (each entry modulo 2^32, as the kernel stores it), *total by the sum of all of them in 64 bits.  n == 0 gives a total of 0. */
int mg_debug_tile_scan(mg_ctx *ctx, uint32_t *x, uint64_t n, uint64_t *total);
/* the scan the three row encoders (mg_format_calls, mg_format_site_info, mg_encode_calls_bcf) run between their length pass and their
 * write pass, on n row lengths of the caller's: row_off_out[0 .. n] receives the exclusive prefix in 64 bits (row_off_out[n] the sum),
 * *total what the encoder would read as the bytes needed.  flag != 0 raises the mark a length pass leaves for a row of 4 GB or more:
 * row_off_out is what it is without the mark, *total is ~0.  n == 0 gives row_off_out[0] = 0 and a total of 0.  No kernel of its own. */
int mg_debug_row_scan(mg_ctx *ctx, const uint32_t *len, uint64_t n, int flag, uint64_t *row_off_out /* [n + 1] */, uint64_t *total);
/* the filter's directory inside the records as the call-time lookups read it: for each slot idx[i] of `bf` (MG_BF_ALT), the
 * counter index (rank) of its bit or -1 when the bit is clear, and the u16 counter the genotyping would read (0 when clear),
 * through the context's current views -- so the counters come from the records' copies whenever those are live.
 * MG_ERR_STATE unless `bf` is finalised, MG_ERR_ARG for a slot at or beyond the filter's size. */
int mg_debug_bucket_count(mg_ctx *ctx, const uint64_t *idx, uint64_t n, int64_t *rank_out, uint32_t *count_out);
/* timing of the first chunk of the most recent mg_kmc_scan* in milliseconds (HIP
 * events on the context's stream): ms_out[0] filter kernel, [1] probe kernel,
 * [2] hit kernel (with the ticket form [0] is its two passes together); rows_out[0] = rows that passed the gate (last chunk),
 * rows_out[1] = rows whose bf bit was set (whole call) */
int mg_scan_stats(mg_ctx *ctx, float *ms_out, uint64_t *rows_out);
/* timing and counts of the most recent mg_cover_blocks_device (waits for it): ms_out[0] tier 1 (classification + the
 * lone-variant lookups), [1] tier 2 (the flat pipeline: chain walks, distinct picks, one thread per signature k-mer), [2] tier 3
 * (the workgroup-per-record kernel on what tier 2 handed on) + the final pass; counts_out[0] records beyond tier 1, [1] signature
 * k-mers of the lone records, [2] signature k-mers tiers 2 and 3 assembled, [3] records tier 3 took */
int mg_blocks_stats(mg_ctx *ctx, float *ms_out, uint64_t *counts_out);
/* 0 disables the cache-resident summary bitmaps (A/B switch; results identical) */
int mg_set_option(mg_ctx *ctx, const char *name, int64_t value);
/* reads an option back, plus "pregate_k" (0: single-level gate), "scan_bins" (slices the
 * most recent scan partitioned its second level into; 0: direct form), "scan_tickets" (gate slices the most
 * recent scan filed tickets under; 0: it did not) and "scan_spilled" */
int mg_get_option(mg_ctx *ctx, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* MALVA_HIP_H */
