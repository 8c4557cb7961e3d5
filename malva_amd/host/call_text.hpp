// A batch of `call` once the device has answered: the per-sample VCF lines (output_variants, var_block.hpp:337-396), the merged output's lines and BCF records
#pragma once
#include "bcf_out.hpp"
#include "panel_batch.hpp"

namespace malva {

// every record's line of every plane pl of P, appended to outs[pl] (a batch's results are [plane][record], [plane][allele slot], [plane][genotype slot])
inline void per_sample_lines(std::vector<std::string> &outs, const std::vector<Rec> &recs, const Batch &iso, const Batch &gen, size_t P, bool haploid, bool verbose, unsigned max_coverage)
{
    const std::string best_default = haploid ? "0" : "0/0";
    auto gname = [&](int a, int c) { return haploid ? std::to_string(a) : std::to_string(a) + "/" + std::to_string(c); };
    char num[64];
    for (const Rec &r : recs)
      for (size_t pl = 0; pl < P; ++pl) {
        const Batch &b = r.isolated ? iso : gen;
        std::string &out = outs[pl];
        const size_t bn = b.n(), bna = b.var_allele_off.back(), bng = b.probs.size() / P;
        out += r.prefix;
        out += "\tPASS\t";
        const uint32_t *cov = &b.cov[pl * bna + r.allele0];
        const uint8_t st = b.status[pl * bn + r.slot];
        if (verbose) {
            out += "COVS=";
            for (uint32_t a = 0; a < r.n_alleles; ++a) {
                out += std::to_string((int)cov[a]);
                out += a + 1 < r.n_alleles ? "," : "";
            }
            out += ";GTS=";
            if (st == MG_GT_NORMAL) {
                size_t q = pl * bng + r.gt0;
                bool first = true;
                for (uint32_t a = 0; a < r.n_alleles; ++a)
                    for (uint32_t c = a; c < (haploid ? a + 1 : r.n_alleles); ++c, ++q) {
                        if (std::isnan(b.probs[q])) snprintf(num, sizeof num, "-nan"); // 0.0/0.0 on x86, as the reference prints it
                        else snprintf(num, sizeof num, "%f", b.probs[q]);               // std::to_string(double)
                        out += (first ? "" : ",") + gname((int)a, (int)c) + ":" + num;
                        first = false;
                    }
            } else {
                // early-outs: one (best_geno, 0) per over-covered allele, or a single entry; 0/0 prints -nan
                size_t entries = 1;
                if (st == MG_GT_OVERCOV) {
                    entries = 0;
                    for (uint32_t a = 0; a < r.n_alleles; ++a) entries += (int)cov[a] > (int)max_coverage;
                }
                for (size_t e = 0; e < entries; ++e) out += (e ? "," : "") + best_default + (st == MG_GT_SINGLE ? ":1.000000" : ":-nan");
            }
        } else
            out += ".";
        out += "\tGT:GQ\t";
        out += gname(b.g1[pl * bn + r.slot], b.g2[pl * bn + r.slot]); // early-outs and "nothing beats 0.0" come back as 0 / 0/0
        out += ":" + std::to_string(b.gq[pl * bn + r.slot]) + "\n";
      }
}

// --merged as text: the fixed columns (the first group's block; INFO from info_text when info_here, else '.') and the sample columns ([0]: of the lone records, [1]: the others)
inline void merged_text_lines(std::string &out, const std::vector<Rec> &recs, const std::vector<char> *row_text, const std::vector<uint64_t> *row_off,
                              const std::vector<char> *info_text, const std::vector<uint64_t> *info_off, bool verbose, bool gp, bool fixed_columns, bool info_here,
                              bool pl = false)
{
    const std::string fixed_text = std::string("\tPASS\t.\tGT:GQ") + (verbose ? ":COVS" : "") + (gp ? ":GP" : "") + (pl ? ":PL" : "");
    const char *fixed = fixed_text.c_str();
    for (const Rec &r : recs) {
        const int w = r.isolated ? 0 : 1;
        if (fixed_columns && info_here) {
            out += r.prefix;
            out += "\tPASS\t";
            out.append(info_text[w].data() + info_off[w][r.slot], info_text[w].data() + info_off[w][r.slot + 1]);
            out += fixed + 7; // (behind "\tPASS\t.")
        } else if (fixed_columns) {
            out += r.prefix;
            out += fixed;
        }
        out.append(row_text[w].data() + row_off[w][r.slot], row_text[w].data() + row_off[w][r.slot + 1]);
    }
}

// --merged as BCF.  direct (one group): whole records -- l_shared, l_indiv, the shared block with INFO from the counts, the device's row --,
// compressed here when bgzf; else the first group's shared block without INFO and every group's row, each behind its u32 length (the paste pass joins them)
inline void merged_bcf_records(std::string &out, const std::vector<Rec> &recs, const std::vector<char> *row_text, const std::vector<uint64_t> *row_off,
                               const std::vector<uint32_t> *site_ac, const std::vector<uint32_t> *site_ns, const BcfHeader &hdr, uint32_t n_fmt, uint32_t planes,
                               bool fixed_columns, bool direct, bool tags, bool bgzf)
{
    std::string plain;
    std::string &rec_out = direct && bgzf ? plain : out;
    for (const Rec &r : recs) {
        const int w = r.isolated ? 0 : 1;
        const char *row = row_text[w].data() + row_off[w][r.slot];
        const uint32_t l_indiv = (uint32_t)(row_off[w][r.slot + 1] - row_off[w][r.slot]);
        if (fixed_columns) {
            const size_t at = rec_out.size();
            rec_out.append(direct ? 8 : 4, '\0');
            bcf_put_shared(rec_out, hdr, r.prefix, n_fmt, direct ? planes : 0);
            if (direct && tags) bcf_put_info(rec_out, at + 8, hdr, site_ac[w].data() + r.allele0, r.n_alleles, site_ns[w][r.slot]);
            const uint32_t l_shared = (uint32_t)(rec_out.size() - at - (direct ? 8 : 4));
            memcpy(&rec_out[at], &l_shared, 4);
            if (direct) memcpy(&rec_out[at + 4], &l_indiv, 4);
        }
        if (!direct) bcf_put_u32(rec_out, l_indiv);
        rec_out.append(row, l_indiv);
    }
    if (direct && bgzf) bgzf_append(plain.data(), plain.size(), out);
}

} // namespace malva
