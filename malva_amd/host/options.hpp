// What the command line of malva-geno says, once parsed (parse_arguments, main.cpp)
#pragma once
#include <cstdint>
#include <string>

#include "cohort_priors.hpp"

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
    bool pl_cap_given = false;
    int32_t pl_cap = 255;   // --pl-cap: the largest PL written (the bcftools convention)
    std::string pairs;      // --pairs: the table of pairwise genotype sharing
    std::string sample_stats; // --sample-stats: the per-sample QC table
    std::string site_stats; // --site-stats: the per-record QC table
    std::string ld;         // --ld: the table of r2 between nearby records
    bool ld_sub = false;    // one of --ld's sub-options was given
    uint32_t ld_window = 64;        // --ld-window: the records behind a record that are its partners (1..MG_LD_MAX_WINDOW)
    uint64_t ld_window_bp = 1000000; // --ld-window-bp: and no further away than this (0: no limit)
    double ld_min_r2 = 0.2;         // --ld-min-r2: the smallest r2 written
    uint32_t ld_min_n = 2;          // --ld-min-n: the fewest samples a pair's r2 is formed from
    std::string ibd;        // --ibd: the table of IBS0-free segments per pair of samples
    bool ibd_sub = false;   // one of --ibd's sub-options was given
    uint32_t ibd_min_records = 100;   // --ibd-min-records: the fewest records of a segment written
    uint64_t ibd_min_bp = 1000000;    // --ibd-min-bp: and its smallest END - START (0: no limit)
    std::string grm;        // --grm: the genetic relationship matrix of the cohort's samples
    bool grm_sub = false;   // one of --grm's sub-options was given
    uint32_t grm_maf_ppm = 10000;     // --grm-min-maf: the smallest minor allele frequency of a record that enters, in parts per million
    uint32_t grm_min_n = 2;           // --grm-min-n: the fewest called samples of a record that enters
    bool grm_gcta = false;            // --grm-format gcta: PATH.grm.bin, PATH.grm.N.bin, PATH.grm.id instead of the text
    PriorOptions priors;    // --cohort-priors and its sub-options (host/cohort_priors.hpp)
};

} // namespace malva
