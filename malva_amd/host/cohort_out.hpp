// cohort_out.hpp -- the host-only half of the outputs of `call --cohort`: the streams a group leaves for the passes behind the last group
// (the records' site counts, the packed calls, the records' genotype counts, the records' site words -- one stream for the LD table, the IBD table and the GRM), the two paste passes over the groups'
// blocks of the merged output, and the text of the --pairs, --sample-stats, --site-stats, --ld, --ibd and --grm tables.  No device is needed: what needs one comes in as a callable (tools/cohort_out_host_check.cpp, tools/site_table_host_check.cpp
// tools/ld_out_host_check.cpp, tools/ibd_out_host_check.cpp and tools/grm_out_host_check.cpp drive this file alone).
#pragma once
#include <deque>
#include <numeric>

#include "../../include/malva_hip.h" // (the MG_SS_* slots of the sample table; nothing here calls the library)
#include "bcf_out.hpp"
#include "part_file.hpp"

namespace malva {

// the groups' scratch files, open for reading as long as this object lives
struct GroupFiles {
    std::vector<FILE *> f;
    GroupFiles() = default;
    GroupFiles(const GroupFiles &) = delete;
    ~GroupFiles() { for (FILE *in : f) fclose(in); }
    void open(const std::string &path)
    {
        FILE *in = fopen(path.c_str(), "rb");
        if (!in) throw std::runtime_error("cannot read " + path);
        f.push_back(in);
    }
    void open(const std::deque<PartFile> &files) { for (const auto &p : files) open(p.path); }
};

// ---- the records' site counts (--site-tags in several groups) ---------------------------------------------------------------------
// per record, in output order, the u32s n_alleles, ns, ac[n_alleles]
inline void put_site_counts(std::string &out, uint32_t n_alleles, uint32_t ns, const uint32_t *ac)
{
    const uint32_t head[2] = {n_alleles, ns};
    out.append((const char *)head, 8);
    out.append((const char *)ac, 4 * (size_t)n_alleles);
}
// the groups' streams read in step and summed
struct SiteCountsReader {
    GroupFiles in;
    std::vector<uint32_t> more;
    const char *short_file = "internal: a group's counts for the merged output are short";
    explicit SiteCountsReader(const std::deque<PartFile> &files) { in.open(files); }
    // the next record: its alleles, the groups' ns summed, their ac summed and appended to `ac`; false where the first group's file ends
    bool next(uint32_t &n_alleles, uint32_t &ns, std::vector<uint32_t> &ac)
    {
        uint32_t head[2], h[2];
        if (fread(head, 4, 2, in.f[0]) != 2) return false;
        const size_t A = head[0], at = ac.size();
        ac.resize(at + A);
        if (A && fread(&ac[at], 4, A, in.f[0]) != A) throw std::runtime_error(short_file);
        more.resize(A);
        for (size_t gi = 1; gi < in.f.size(); ++gi) {
            if (fread(h, 4, 2, in.f[gi]) != 2 || h[0] != A || (A && fread(more.data(), 4, A, in.f[gi]) != A)) throw std::runtime_error(short_file);
            head[1] += h[1];
            for (size_t a = 0; a < A; ++a) ac[at + a] += more[a];
        }
        n_alleles = head[0];
        ns = head[1];
        return true;
    }
    // up to `most` records as mg_format_site_info takes them (var_allele_off starts at 0); at least one, or the streams are short
    void next_batch(size_t most, std::vector<uint32_t> &ac, std::vector<uint32_t> &ns, std::vector<uint32_t> &var_allele_off)
    {
        ac.clear();
        ns.clear();
        var_allele_off.assign(1, 0u);
        uint32_t A, n;
        while (ns.size() < most && next(A, n, ac)) {
            ns.push_back(n);
            var_allele_off.push_back((uint32_t)ac.size());
        }
        if (ns.empty()) throw std::runtime_error(short_file);
    }
};

// ---- the packed calls (--pairs in several groups) ---------------------------------------------------------------------------------
// per batch and stream the u64s stream, n_records, then the [planes][3][W] words of mg_pack_dosage, W = ceil(n_records / 64)
inline void put_pack_batch(std::string &out, uint64_t stream, uint64_t n_records, const std::vector<uint64_t> &words)
{
    const uint64_t head[2] = {stream, n_records};
    out.append((const char *)head, 16);
    out.append((const char *)words.data(), 8 * words.size());
}
// Two groups' files walked in step: every group saw the records in the same order and cut them into the same batches, so batch b of
// the one and batch b of the other hold the same records.  count(W, words_a, words_b) gets each pair of batches.
template <class Count> void walk_pack_pair(const std::string &path_a, size_t planes_a, const std::string &path_b, size_t planes_b, Count &&count)
{
    const char *short_file = "internal: a group's packed calls for the pair table are short";
    GroupFiles in;
    in.open(path_a);
    in.open(path_b);
    FILE *fa = in.f[0], *fb = in.f[1];
    std::vector<uint64_t> words_a, words_b;
    uint64_t head_a[2], head_b[2];
    while (fread(head_a, 8, 2, fa) == 2) {
        if (fread(head_b, 8, 2, fb) != 2 || head_b[0] != head_a[0] || head_b[1] != head_a[1]) throw std::runtime_error(short_file);
        const size_t W = (size_t)((head_a[1] + 63) / 64);
        words_a.resize(planes_a * 3 * W);
        words_b.resize(planes_b * 3 * W);
        if (fread(words_a.data(), 8, words_a.size(), fa) != words_a.size() || fread(words_b.data(), 8, words_b.size(), fb) != words_b.size())
            throw std::runtime_error(short_file);
        count(W, words_a.data(), words_b.data());
    }
    if (fread(head_b, 8, 2, fb) != 0) throw std::runtime_error(short_file);
}

// ---- the tables' text: the divisions and the formatting are all the host does ------------------------------------------------------
// table: [samples][samples][9], of which the entries i < j are read
inline std::string pair_table_text(const std::vector<std::string> &names, const uint64_t *table)
{
    std::string text = "#A\tB\tN\tN00\tN01\tN02\tN10\tN11\tN12\tN20\tN21\tN22\tIBS0\tIBS1\tIBS2\tKING\n";
    char num[64];
    const size_t S = names.size();
    for (size_t i = 0; i < S; ++i)
        for (size_t j = i + 1; j < S; ++j) {
            const uint64_t *c = &table[(i * S + j) * 9];
            uint64_t total = 0;
            for (int k = 0; k < 9; ++k) total += c[k];
            const uint64_t ibs2 = c[0] + c[4] + c[8], ibs0 = c[2] + c[6], het = (c[3] + c[4] + c[5]) + (c[1] + c[4] + c[7]);
            text += names[i] + "\t" + names[j] + "\t" + std::to_string(total);
            for (int k = 0; k < 9; ++k) text += "\t" + std::to_string(c[k]);
            text += "\t" + std::to_string(ibs0) + "\t" + std::to_string(total - ibs0 - ibs2) + "\t" + std::to_string(ibs2) + "\t";
            if (het) {
                snprintf(num, sizeof num, "%.4f", (double)((int64_t)c[4] - 2 * (int64_t)ibs0) / (double)het);
                text += num;
            } else
                text += ".";
            text += "\n";
        }
    return text;
}
// table: [samples][MG_SAMPLE_SLOTS]
inline std::string sample_table_text(const std::vector<std::string> &names, const uint64_t *table)
{
    std::string text = "#SAMPLE\tRECORDS\tCALLED\tMASKED\tBAD\tHOM_REF\tHET\tHOM_ALT\tHET_ALT\tTS\tTV\tINS\tDEL\tOTHER\tGQ_SUM\tCOV_SUM\tNORMAL\tOVERCOV\tSINGLE\tNOCOV";
    for (int b = 0; b < 10; ++b) text += "\tGQ_" + std::to_string(10 * b);
    text += "\tCALL_RATE\tHET_HOM\tTSTV\tMEAN_GQ\tMEAN_COV\n";
    char num[64];
    for (size_t i = 0; i < names.size(); ++i) {
        const uint64_t *c = &table[i * MG_SAMPLE_SLOTS];
        text += names[i];
        for (int k : {MG_SS_RECORDS, MG_SS_CALLED, MG_SS_MASKED, MG_SS_BAD, MG_SS_HOM_REF, MG_SS_HET, MG_SS_HOM_ALT, MG_SS_HET_ALT, MG_SS_TS, MG_SS_TV, MG_SS_INS,
                      MG_SS_DEL, MG_SS_OTHER})
            text += "\t" + std::to_string(c[k]);
        text += "\t" + std::to_string((int64_t)c[MG_SS_GQ_SUM]);
        for (int k = MG_SS_COV_SUM; k < MG_SS_COUNTED; ++k) text += "\t" + std::to_string(c[k]);
        const double ratio[5][2] = {{(double)c[MG_SS_CALLED], (double)c[MG_SS_RECORDS]},
                                    {(double)c[MG_SS_HET], (double)c[MG_SS_HOM_ALT]},
                                    {(double)c[MG_SS_TS], (double)c[MG_SS_TV]},
                                    {(double)(int64_t)c[MG_SS_GQ_SUM], (double)c[MG_SS_CALLED]},
                                    {(double)c[MG_SS_COV_SUM], (double)c[MG_SS_RECORDS]}};
        for (const auto &r : ratio) {
            if (r[1] != 0) {
                snprintf(num, sizeof num, "\t%.4f", r[0] / r[1]);
                text += num;
            } else
                text += "\t.";
        }
        text += "\n";
    }
    return text;
}

// ---- the per-record table (--site-stats) ------------------------------------------------------------------------------------------
// One line per record with an ALT: the record's first five columns, SAMPLES (the cohort), N (the usable cells: mg_site_geno_counts), AN, and a
// comma list per ALT of AC, AF, HOM, HET, HWE, EXC_HET (mg_hwe_exact).  Diploid: AN = 2 N, AC = het + 2 hom; haploid: AN = N, AC = hom.
inline const char *site_stats_header() { return "#CHROM\tPOS\tID\tREF\tALT\tSAMPLES\tN\tAN\tAC\tAF\tHOM\tHET\tHWE\tEXC_HET\n"; }
// how much of a record's fixed columns (CHROM .. QUAL, as Rec::prefix holds them) the first five are
inline size_t site_stats_cols(const std::string &prefix)
{
    size_t at = 0;
    for (int t = 0; t < 5 && at != std::string::npos; ++t) at = prefix.find('\t', at + (t ? 1 : 0));
    return at == std::string::npos ? prefix.size() : at;
}
// AF by the integer rule of mg_format_site_info: six decimals rounded half up, trailing zeros dropped, `0`, `1`, `.` when AN = 0
inline void site_stats_af(std::string &out, uint64_t ac, uint64_t an)
{
    if (an == 0) {
        out += '.';
        return;
    }
    uint64_t q = (2 * ac * 1000000 + an) / (2 * an);
    if (q == 0 || q >= 1000000) {
        out += q ? '1' : '0';
        return;
    }
    char digits[8];
    snprintf(digits, sizeof digits, "%06u", (unsigned)q);
    size_t nd = 6;
    while (digits[nd - 1] == '0') --nd;
    out += "0.";
    out.append(digits, nd);
}
// the items of mg_hwe_exact a record gives, one per ALT, appended
inline void site_stats_items(uint32_t n_alleles, uint32_t n, const uint32_t *het, const uint32_t *hom, std::vector<uint32_t> &item_n, std::vector<uint32_t> &item_het,
                             std::vector<uint32_t> &item_hom)
{
    for (uint32_t a = 1; a < n_alleles; ++a) item_n.push_back(n), item_het.push_back(het[a]), item_hom.push_back(hom[a]);
}
// the record's line (none for a record without ALT).  het / hom: its n_alleles slots; hwe / exc: its n_alleles - 1 values, not read in haploid mode
inline void site_stats_row(std::string &out, const char *cols, size_t cols_len, size_t samples, bool haploid, uint32_t n_alleles, uint32_t n, const uint32_t *het,
                           const uint32_t *hom, const double *hwe, const double *exc)
{
    if (n_alleles < 2) return;
    const uint64_t an = haploid ? n : 2 * (uint64_t)n;
    out.append(cols, cols_len);
    out += "\t" + std::to_string(samples) + "\t" + std::to_string(n) + "\t" + std::to_string(an);
    auto list = [&](auto &&item) {
        out += '\t';
        for (uint32_t a = 1; a < n_alleles; ++a) {
            if (a > 1) out += ',';
            item(a);
        }
    };
    auto ac = [&](uint32_t a) { return haploid ? (uint64_t)hom[a] : het[a] + 2 * (uint64_t)hom[a]; };
    auto p_value = [&](const double *p, uint32_t a) {
        char num[40];
        if (haploid || n == 0) out += '.';
        else {
            snprintf(num, sizeof num, "%.6g", p[a - 1]);
            out += num;
        }
    };
    list([&](uint32_t a) { out += std::to_string(ac(a)); });
    list([&](uint32_t a) { site_stats_af(out, ac(a), an); });
    list([&](uint32_t a) { out += std::to_string(hom[a]); });
    list([&](uint32_t a) { out += std::to_string(het[a]); });
    list([&](uint32_t a) { p_value(hwe, a); });
    list([&](uint32_t a) { p_value(exc, a); });
    out += '\n';
}

// The cohort in several groups: every group leaves per record, in output order, the u32s n_alleles, n, het[n_alleles], hom[n_alleles]; the first
// group's stream has behind each record a u32 length and that many bytes, the record's first five columns.
inline void put_site_geno(std::string &out, uint32_t n_alleles, uint32_t n, const uint32_t *het, const uint32_t *hom, const char *cols, size_t cols_len)
{
    const uint32_t head[2] = {n_alleles, n};
    out.append((const char *)head, 8);
    out.append((const char *)het, 4 * (size_t)n_alleles);
    out.append((const char *)hom, 4 * (size_t)n_alleles);
    if (!cols) return;
    const uint32_t len = (uint32_t)cols_len;
    out.append((const char *)&len, 4);
    out.append(cols, cols_len);
}
// the groups' streams read in step and summed
struct SiteGenoReader {
    GroupFiles in;
    std::vector<uint32_t> more;
    const char *short_file = "internal: a group's counts for the per-record table are short";
    explicit SiteGenoReader(const std::deque<PartFile> &files) { in.open(files); }
    // the next record: its alleles, the groups' n summed, their het and hom summed and appended, its columns; false where the first group's file ends
    bool next(uint32_t &n_alleles, uint32_t &n, std::vector<uint32_t> &het, std::vector<uint32_t> &hom, std::string &cols)
    {
        uint32_t head[2], h[2], len;
        if (fread(head, 4, 2, in.f[0]) != 2) return false;
        const size_t A = head[0], at = het.size();
        if (hom.size() != at) throw std::logic_error("SiteGenoReader: het and hom differ in length");
        het.resize(at + A);
        hom.resize(at + A);
        if (A && (fread(&het[at], 4, A, in.f[0]) != A || fread(&hom[at], 4, A, in.f[0]) != A)) throw std::runtime_error(short_file);
        if (fread(&len, 4, 1, in.f[0]) != 1) throw std::runtime_error(short_file);
        cols.resize(len);
        if (len && fread(&cols[0], 1, len, in.f[0]) != len) throw std::runtime_error(short_file);
        more.resize(A);
        for (size_t gi = 1; gi < in.f.size(); ++gi) {
            if (fread(h, 4, 2, in.f[gi]) != 2 || h[0] != A) throw std::runtime_error(short_file);
            head[1] += h[1];
            for (std::vector<uint32_t> *sum : {&het, &hom}) {
                if (A && fread(more.data(), 4, A, in.f[gi]) != A) throw std::runtime_error(short_file);
                for (size_t a = 0; a < A; ++a) (*sum)[at + a] += more[a];
            }
        }
        n_alleles = head[0];
        n = head[1];
        return true;
    }
    // behind the last record every later group's stream must have ended too
    void end()
    {
        char one;
        for (size_t gi = 1; gi < in.f.size(); ++gi)
            if (fread(&one, 1, 1, in.f[gi]) != 0) throw std::runtime_error(short_file);
    }
};
// The pass behind the last group: the header, then the records' lines, `batch` records at a time -- their items go to
// hwe(n_items, n, het, hom, hwe_out, exc_out) (mg_hwe_exact, whoever holds the device; not called in haploid mode), the text to sink(data, n).
template <class Hwe, class Sink> void site_stats_groups(const std::deque<PartFile> &files, size_t samples, bool haploid, size_t batch, Hwe &&hwe, Sink &&sink)
{
    SiteGenoReader in(files);
    std::string out = site_stats_header();
    std::vector<uint32_t> A, n, het, hom, item_n, item_het, item_hom;
    std::vector<std::string> cols;
    std::vector<double> p, exc;
    for (bool more = true; more;) {
        A.clear(), n.clear(), het.clear(), hom.clear(), item_n.clear(), item_het.clear(), item_hom.clear();
        size_t nr = 0;
        for (uint32_t a, nn; nr < batch; ++nr) {
            if (cols.size() <= nr) cols.emplace_back();
            if (!(more = in.next(a, nn, het, hom, cols[nr]))) break;
            A.push_back(a), n.push_back(nn);
            if (!haploid) site_stats_items(a, nn, het.data() + het.size() - a, hom.data() + hom.size() - a, item_n, item_het, item_hom);
        }
        p.resize(item_n.size()), exc.resize(item_n.size());
        if (!item_n.empty()) hwe(item_n.size(), item_n.data(), item_het.data(), item_hom.data(), p.data(), exc.data());
        for (size_t r = 0, slot = 0, item = 0; r < nr; slot += A[r], item += haploid || !A[r] ? 0 : A[r] - 1, ++r)
            site_stats_row(out, cols[r].data(), cols[r].size(), samples, haploid, A[r], n[r], het.data() + slot, hom.data() + slot, p.data() + item, exc.data() + item);
        sink(out.data(), out.size());
        out.clear();
    }
    in.end();
}

// ---- the records' site words (--ld, --ibd, --grm) ---------------------------------------------------------------------------------
// Every group -- a cohort of one group too -- leaves per record, in output order, the three u64 words of mg_pack_site_dosage over its planes and the
// u32 n_alleles; the first group's stream has behind each record a u32 length and that many bytes, the record's first five columns.  One stream per
// group serves the three tables: each of their passes behind the last group reads it with a reader of its own.
inline void put_site_words(std::string &out, uint64_t w0, uint64_t w1, uint64_t w2, uint32_t n_alleles, const char *cols, size_t cols_len)
{
    const uint64_t w[3] = {w0, w1, w2};
    out.append((const char *)w, 24);
    out.append((const char *)&n_alleles, 4);
    if (!cols) return;
    const uint32_t len = (uint32_t)cols_len;
    out.append((const char *)&len, 4);
    out.append(cols, cols_len);
}
// The groups' streams read in step.  The reader holds a run of records: words [record][group][3], the records' CHROM\tPOS\tID, a running contig
// id that steps whenever the CHROM text changes, and POS parsed.
struct SiteWordsReader {
    GroupFiles in;
    size_t G;
    std::vector<uint64_t> words;
    std::vector<std::string> cols;
    std::vector<size_t> pos_at; // where POS starts in cols
    std::vector<uint32_t> chrom, pos;
    std::string last_chrom, five;
    uint32_t chrom_id = 0;
    bool any = false, ended = false;
    const char *const short_file; // the pass's own text: "internal: a group's words for the ... are short"
    SiteWordsReader(const std::deque<PartFile> &files, const char *short_file) : short_file(short_file)
    {
        in.open(files);
        G = in.f.size();
        if (!G) throw std::logic_error("SiteWordsReader: no group");
    }
    size_t held() const { return cols.size(); }
    // one more record behind those held; false where the first group's stream ends (every later group's must end there too)
    bool read_one()
    {
        if (ended) return false;
        const size_t at = words.size();
        words.resize(at + 3 * G);
        uint32_t A, a, len;
        const size_t got = fread(&words[at], 8, 3, in.f[0]);
        if (got == 0) {
            char one;
            for (size_t gi = 1; gi < G; ++gi)
                if (fread(&one, 1, 1, in.f[gi]) != 0) throw std::runtime_error(short_file);
            words.resize(at);
            ended = true;
            return false;
        }
        if (got != 3 || fread(&A, 4, 1, in.f[0]) != 1 || fread(&len, 4, 1, in.f[0]) != 1) throw std::runtime_error(short_file);
        five.resize(len);
        if (len && fread(&five[0], 1, len, in.f[0]) != len) throw std::runtime_error(short_file);
        for (size_t gi = 1; gi < G; ++gi)
            if (fread(&words[at + 3 * gi], 8, 3, in.f[gi]) != 3 || fread(&a, 4, 1, in.f[gi]) != 1 || a != A) throw std::runtime_error(short_file);
        size_t tab[3] = {0, 0, 0};
        for (int t = 0; t < 3; ++t) {
            tab[t] = five.find('\t', t ? tab[t - 1] + 1 : 0);
            if (tab[t] == std::string::npos) {
                if (t < 2) throw std::runtime_error("internal: a record's columns in the LD table's stream are short");
                tab[t] = five.size();
            }
        }
        if (!any || five.compare(0, tab[0], last_chrom) != 0) {
            if (any) ++chrom_id;
            last_chrom.assign(five, 0, tab[0]);
            any = true;
        }
        chrom.push_back(chrom_id);
        pos.push_back((uint32_t)strtoul(five.c_str() + tab[0] + 1, nullptr, 10));
        pos_at.push_back(tab[0] + 1);
        cols.emplace_back(five, 0, tab[2]);
        return true;
    }
    // the first n records leave
    void drop(size_t n)
    {
        words.erase(words.begin(), words.begin() + 3 * G * n);
        cols.erase(cols.begin(), cols.begin() + n);
        pos_at.erase(pos_at.begin(), pos_at.begin() + n);
        chrom.erase(chrom.begin(), chrom.begin() + n);
        pos.erase(pos.begin(), pos.begin() + n);
    }
    // the held records as mg_ld_window takes them: [G][3][held]
    void sites(std::vector<uint64_t> &out) const
    {
        const size_t n = held();
        out.resize(3 * G * n);
        for (size_t v = 0; v < n; ++v)
            for (size_t k = 0; k < 3 * G; ++k) out[k * n + v] = words[v * 3 * G + k];
    }
};
inline size_t cohort_size(const std::vector<size_t> &group_sizes) { return std::accumulate(group_sizes.begin(), group_sizes.end(), (size_t)0); }
// The records held by a reader over groups of group_sizes[g] samples (bits 0 .. size - 1 of a group's words) as mg_ibd_step and mg_grm_step take
// them: the cohort's samples side by side, sample s in bit s & 63 of word s >> 6, [ceil(S / 64)][3][held] -- whatever the grouping was.
inline void cohort_sites(const SiteWordsReader &in, const std::vector<size_t> &group_sizes, std::vector<uint64_t> &out)
{
    const size_t n = in.held(), W = (cohort_size(group_sizes) + 63) / 64;
    out.assign(3 * W * n, 0);
    for (size_t v = 0; v < n; ++v) {
        size_t s0 = 0;
        for (size_t gi = 0; gi < in.G; ++gi) {
            const size_t g = group_sizes[gi], word = s0 >> 6, bit = s0 & 63;
            const uint64_t mask = g >= 64 ? ~0ull : (1ull << g) - 1;
            for (size_t d = 0; d < 3; ++d) {
                const uint64_t w = in.words[(v * in.G + gi) * 3 + d] & mask;
                out[(word * 3 + d) * n + v] |= w << bit;
                if (bit && bit + g > 64) out[((word + 1) * 3 + d) * n + v] |= w >> (64 - bit);
            }
            s0 += g;
        }
    }
}
// The front of the two passes without look-ahead (ibd_table and grm_table; `who` starts their logic errors): the reader's streams walked `chunk` records
// at a time.  each(sites, ended, in) gets a chunk's cohort_sites and whether the streams have ended; the reader still holds the chunk (held(), cols,
// chrom, pos), which is dropped behind the call.  The last call is the one with `ended` set: its chunk is empty where the records end on a chunk's edge.
template <class Each> void walk_cohort_sites(SiteWordsReader &in, const std::vector<size_t> &group_sizes, size_t chunk, const std::string &who, Each &&each)
{
    for (const size_t g : group_sizes)
        if (g < 1 || g > 64) throw std::logic_error(who + ": a group of 1..64 samples");
    if (!chunk || group_sizes.size() != in.G) throw std::logic_error(who + ": an empty chunk, or groups that are not the streams'");
    std::vector<uint64_t> sites;
    do {
        while (in.held() < chunk && in.read_one()) {}
        cohort_sites(in, group_sizes, sites);
        each(sites, in.ended, in);
        in.drop(in.held());
    } while (!in.ended);
}

// ---- the LD table (--ld) -------------------------------------------------------------------------------------------------------
// One line per emitted pair of records (mg_ld_window): A's CHROM, POS and ID, B's POS and ID, N (the samples that contribute in both), R2 to six
// significant digits and the sign of the covariance.  Lines are in the order of the merged output, by A, then by B.
inline const char *ld_header() { return "#CHROM\tPOS_A\tID_A\tPOS_B\tID_B\tN\tR2\tSIGN\n"; }
inline void ld_row(std::string &out, const std::string &a, const std::string &b, size_t b_pos_at, const mg_ld_pair &p)
{
    char num[64];
    out += a;
    out += '\t';
    out.append(b, b_pos_at, std::string::npos);
    snprintf(num, sizeof num, "\t%u\t%.6g\t%c\n", p.n, p.r2, p.sign > 0 ? '+' : p.sign < 0 ? '-' : '0');
    out += num;
}
// The pass behind the last group: the header, then the pairs' lines, `chunk` records at a time with a look-ahead of `window` records that become the
// head of the next chunk.  ld(n_vars, n_first, n_groups, sites, chrom, pos, pairs_out, pairs_cap, row_off_out, n_pairs_out) is mg_ld_window with the
// run's options, whoever holds the device: it returns MG_OK or MG_ERR_LIMIT (then the buffer grows and it is called once more).  The text goes
// to sink(data, n).
template <class Ld, class Sink> void ld_table(const std::deque<PartFile> &files, size_t window, size_t chunk, Ld &&ld, Sink &&sink)
{
    SiteWordsReader in(files, "internal: a group's words for the LD table are short");
    std::string out = ld_header();
    std::vector<uint64_t> sites, row_off;
    std::vector<mg_ld_pair> pairs(1024);
    if (!chunk || !window) throw std::logic_error("ld_table: an empty chunk or window");
    for (;;) {
        while (in.held() < chunk + window && in.read_one()) {}
        const size_t n = in.held(), n_first = in.ended ? n : chunk;
        if (n) {
            in.sites(sites);
            row_off.assign(n_first + 1, 0);
            uint64_t needed = 0;
            int rc = ld(n, n_first, in.G, sites.data(), in.chrom.data(), in.pos.data(), pairs.data(), pairs.size(), row_off.data(), &needed);
            if (rc == MG_ERR_LIMIT) {
                pairs.resize(needed);
                rc = ld(n, n_first, in.G, sites.data(), in.chrom.data(), in.pos.data(), pairs.data(), pairs.size(), row_off.data(), &needed);
            }
            if (rc != MG_OK || needed > pairs.size() || row_off[n_first] != needed) throw std::runtime_error("internal: the LD table's pairs do not fit their buffer");
            for (uint64_t k = 0; k < needed; ++k) {
                const mg_ld_pair &p = pairs[k];
                if (p.i >= n_first || p.j >= n || p.j <= p.i) throw std::runtime_error("internal: a pair of the LD table lies outside its chunk");
                ld_row(out, in.cols[p.i], in.cols[p.j], in.pos_at[p.j], p);
            }
        }
        sink(out.data(), out.size());
        out.clear();
        if (in.ended) break;
        in.drop(n_first);
    }
}

// ---- the IBD table (--ibd) ------------------------------------------------------------------------------------------------------
// One line per IBS0-free segment of a pair of samples (mg_ibd_step): the two names, CHROM, START, END, LENGTH = END - START, N and IBS2.  Lines are
// ordered by pair -- A, then B, in the manifest's order -- and along the merged output.
inline const char *ibd_header() { return "#A\tB\tCHROM\tSTART\tEND\tLENGTH\tN\tIBS2\n"; }
inline void ibd_row(std::string &out, const std::string &a, const std::string &b, const std::string &chrom, const mg_ibd_seg &s)
{
    char num[128];
    out += a;
    out += '\t';
    out += b;
    out += '\t';
    out += chrom;
    snprintf(num, sizeof num, "\t%u\t%u\t%lld\t%u\t%u\n", s.start_pos, s.end_pos, (long long)s.end_pos - (long long)s.start_pos, s.n, s.ibs2);
    out += num;
}
// The pass behind the last group: the groups' streams walked `chunk` records at a time (walk_cohort_sites) -- no look-ahead: the pairs' state stays on the
// device between the steps -- the closed segments collected, put into (A, B, along the records) order by a stable sort by (A, B) of the steps' outputs, and written.
// The whole table is held in memory, 32 bytes per segment.  step(n_vars, n_groups, sites, chrom, pos, flush, segs_out, segs_cap, n_segs_out) is
// mg_ibd_step behind an mg_ibd_begin for names.size() samples, whoever holds the device: it returns MG_OK or MG_ERR_LIMIT (then the buffer grows
// and it is called once more; the state has not moved).  A cohort of one sample has no pair: the header alone, and the streams
// are not read.  The text goes to sink(data, n).
template <class Step, class Sink>
void ibd_table(const std::deque<PartFile> &files, const std::vector<size_t> &group_sizes, const std::vector<std::string> &names, size_t chunk, Step &&step, Sink &&sink)
{
    SiteWordsReader reader(files, "internal: a group's words for the IBD table are short");
    const size_t S = names.size();
    if (cohort_size(group_sizes) != S) throw std::logic_error("ibd_table: groups that are not the names'");
    std::string out = ibd_header();
    std::vector<mg_ibd_seg> all, segs(1024);
    std::vector<std::string> chrom_names; // by the reader's running contig id
    if (S >= 2)
        walk_cohort_sites(reader, group_sizes, chunk, "ibd_table", [&](const std::vector<uint64_t> &sites, const int flush, const SiteWordsReader &in) {
            const size_t n = in.held();
            for (size_t v = 0; v < n; ++v)
                if (in.chrom[v] == chrom_names.size()) chrom_names.emplace_back(in.cols[v], 0, in.pos_at[v] - 1);
            uint64_t needed = 0;
            int rc = step(n, (S + 63) / 64, sites.data(), in.chrom.data(), in.pos.data(), flush, segs.data(), segs.size(), &needed);
            if (rc == MG_ERR_LIMIT) {
                segs.resize(needed);
                rc = step(n, (S + 63) / 64, sites.data(), in.chrom.data(), in.pos.data(), flush, segs.data(), segs.size(), &needed);
            }
            if (rc != MG_OK || needed > segs.size()) throw std::runtime_error("internal: the IBD table's segments do not fit their buffer");
            for (uint64_t k = 0; k < needed; ++k) {
                const mg_ibd_seg &s = segs[k];
                if (s.a >= s.b || s.b >= S || s.chrom >= chrom_names.size()) throw std::runtime_error("internal: a segment of the IBD table names no pair or no contig");
            }
            all.insert(all.end(), segs.begin(), segs.begin() + needed);
        });
    std::stable_sort(all.begin(), all.end(), [](const mg_ibd_seg &x, const mg_ibd_seg &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
    for (const mg_ibd_seg &s : all) {
        ibd_row(out, names[s.a], names[s.b], chrom_names[s.chrom], s);
        if (out.size() >= (1u << 20)) {
            sink(out.data(), out.size());
            out.clear();
        }
    }
    sink(out.data(), out.size());
}

// ---- the GRM (--grm) ----------------------------------------------------------------------------------------------------------------
// The genetic relationship matrix (mg_grm_step): per pair of samples a <= b, in the manifest's order, N -- the entering records where both are called --
// and S / (2^20 N).  The text has six decimals, formed in integers: S 10^6 / (2^20 N) rounded half away from zero, no sign on a value that
// rounds to zero, `.` where N is 0.
inline const char *grm_header() { return "#A\tB\tN\tGRM\n"; }
inline void grm_value(std::string &out, int64_t s, uint64_t n)
{
    if (!n) {
        out += '.';
        return;
    }
    const unsigned __int128 mag = s < 0 ? (unsigned __int128)(-(__int128)s) : (unsigned __int128)s, den = (unsigned __int128)n << 20;
    const unsigned __int128 v = (2 * mag * 1000000u + den) / (2 * den);
    char num[64];
    snprintf(num, sizeof num, "%s%llu.%06u", s < 0 && v ? "-" : "", (unsigned long long)(v / 1000000u), (unsigned)(v % 1000000u));
    out += num;
}
struct GrmState { // mg_grm_read's outputs: pair (a, b), a <= b, row-major
    std::vector<int64_t> sum;
    std::vector<uint64_t> n;
    uint64_t records[2] = {0, 0}; // seen, entered
};
// The pass behind the last group: the groups' streams walked `chunk` records at a time (walk_cohort_sites) and every chunk that holds a record
// handed to step(n_vars, n_groups, sites) -- mg_grm_step behind an mg_grm_begin for the groups' samples, whoever holds the device; the pairs' sums
// stay there between the steps.  read(sum, n, records) -- mg_grm_read -- is called once, behind the last step.
template <class Step, class Read> GrmState grm_table(const std::deque<PartFile> &files, const std::vector<size_t> &group_sizes, size_t chunk, Step &&step, Read &&read)
{
    SiteWordsReader reader(files, "internal: a group's words for the GRM are short");
    const size_t S = cohort_size(group_sizes);
    walk_cohort_sites(reader, group_sizes, chunk, "grm_table", [&](const std::vector<uint64_t> &sites, bool, const SiteWordsReader &in) {
        if (in.held()) step(in.held(), (S + 63) / 64, sites.data());
    });
    GrmState st;
    st.sum.resize(S * (S + 1) / 2), st.n.resize(S * (S + 1) / 2);
    read(st.sum.data(), st.n.data(), st.records);
    return st;
}
// the table's text, to sink(data, n) about a MiB at a time
template <class Sink> void grm_text(const GrmState &st, const std::vector<std::string> &names, Sink &&sink)
{
    const size_t S = names.size();
    if (st.sum.size() != S * (S + 1) / 2 || st.n.size() != st.sum.size()) throw std::logic_error("grm_text: a state that is not the names'");
    std::string out = grm_header();
    char num[32];
    for (size_t a = 0, k = 0; a < S; ++a)
        for (size_t b = a; b < S; ++b, ++k) {
            out += names[a];
            out += '\t';
            out += names[b];
            snprintf(num, sizeof num, "\t%llu\t", (unsigned long long)st.n[k]);
            out += num;
            grm_value(out, st.sum[k], st.n[k]);
            out += '\n';
            if (out.size() >= (1u << 20)) {
                sink(out.data(), out.size());
                out.clear();
            }
        }
    sink(out.data(), out.size());
}
// GCTA's binary form: values(data, n), counts(data, n) and ids(data, n) receive the bytes of PATH.grm.bin, PATH.grm.N.bin -- float32, the lower
// triangle row by row, diagonal included: (float)((double)S / ((double)N 1048576.0)), 0 where N is 0, and N as a float -- and PATH.grm.id,
// NAME\tNAME per sample.
template <class Values, class Counts, class Ids> void grm_gcta(const GrmState &st, const std::vector<std::string> &names, Values &&values, Counts &&counts, Ids &&ids)
{
    const size_t S = names.size();
    if (st.sum.size() != S * (S + 1) / 2 || st.n.size() != st.sum.size()) throw std::logic_error("grm_gcta: a state that is not the names'");
    std::vector<float> val, cnt;
    for (size_t i = 0; i < S; ++i) {
        val.resize(i + 1), cnt.resize(i + 1);
        for (size_t j = 0; j <= i; ++j) { // the pair a = j, b = i
            const size_t k = j * (2 * S - j + 1) / 2 + (i - j);
            val[j] = st.n[k] ? (float)((double)st.sum[k] / ((double)st.n[k] * 1048576.0)) : 0.f;
            cnt[j] = (float)st.n[k];
        }
        values((const char *)val.data(), 4 * (i + 1));
        counts((const char *)cnt.data(), 4 * (i + 1));
    }
    std::string id;
    for (const std::string &name : names) id += name + "\t" + name + "\n";
    ids(id.data(), id.size());
}

// ---- the paste passes over the groups' blocks of the merged output -----------------------------------------------------------------
// Both read in[g], group g's block, and hand the output to sink(data, n) about a MiB at a time.
//
// Text: line i of the output = line i of every group's block, one behind the other (the header lines of the first block have no
// counterpart in the others).  site_tags: INFO, the eighth column, is the first block's '.' and is replaced by the next string of
// next_infos(text, off), which hands out the strings of as many records as it likes (off: their n + 1 offsets into text), n >= 1.
template <class Infos, class Sink> void paste_text_groups(const std::vector<FILE *> &in, bool site_tags, Infos &&next_infos, Sink &&sink)
{
    std::vector<char> info_text;
    std::vector<uint64_t> info_off(1, 0);
    size_t info_at = 0;
    char *line = nullptr;
    size_t line_cap = 0;
    struct FreeLine {
        char *&p;
        ~FreeLine() { free(p); }
    } free_line{line};
    std::string out;
    for (;;) {
        ssize_t len = getline(&line, &line_cap, in[0]);
        if (len < 0) break;
        const bool record = line[0] != '#';
        if (record && len && line[len - 1] == '\n') --len;
        if (record && site_tags) {
            if (info_at + 1 == info_off.size()) {
                next_infos(info_text, info_off);
                info_at = 0;
            }
            const char *at = line;
            for (int t = 0; t < 7 && at; ++t) {
                at = (const char *)memchr(at, '\t', (size_t)(line + len - at));
                if (at) ++at;
            }
            if (!at || line + len - at < 2 || at[0] != '.' || at[1] != '\t') throw std::runtime_error("internal: a line of the merged output's first block has no INFO column");
            out.append(line, (size_t)(at - line));
            out.append(info_text.data() + info_off[info_at], info_text.data() + info_off[info_at + 1]);
            out.append(at + 1, (size_t)(line + len - at - 1));
            ++info_at;
        } else
            out.append(line, (size_t)len);
        for (size_t gi = 1; record && gi < in.size(); ++gi) {
            ssize_t more = getline(&line, &line_cap, in[gi]);
            if (more <= 0) throw std::runtime_error("internal: a group's block of the merged output is short");
            if (gi + 1 < in.size() && line[more - 1] == '\n') --more;
            out.append(line, (size_t)more);
        }
        if (out.size() >= (1u << 20)) {
            sink(out.data(), out.size());
            out.clear();
        }
    }
    sink(out.data(), out.size());
}

// BCF: record i of the output = the first group's shared block -- n_fmt and the cohort's n_samples put right, INFO from the summed
// counts when `counts` is given -- and the groups' per-sample blocks joined field by field (bcf_paste_rows: planes[g] samples in
// group g), framed by l_shared and l_indiv.  bgzf: every piece leaves as whole BGZF members, and the empty member ends the stream.
template <class Sink>
void paste_bcf_groups(const std::vector<FILE *> &in, const std::vector<uint32_t> &planes, uint32_t n_fmt, uint32_t n_samples, const BcfHeader &hdr, SiteCountsReader *counts,
                      bool bgzf, Sink &&sink)
{
    if (planes.size() != in.size()) throw std::runtime_error("internal: the groups of the merged output and their files disagree");
    const char *short_file = "internal: a group's block of the merged output is short";
    std::vector<std::vector<unsigned char>> rows(in.size());
    std::vector<std::pair<const unsigned char *, size_t>> row_of(in.size());
    std::vector<uint32_t> ac;
    std::string out, shared, indiv;
    auto flush = [&]() {
        std::string packed;
        if (bgzf) bgzf_append(out.data(), out.size(), packed);
        const std::string &bytes = bgzf ? packed : out;
        sink(bytes.data(), bytes.size());
        out.clear();
    };
    for (;;) {
        uint32_t l_shared;
        if (fread(&l_shared, 4, 1, in[0]) != 1) break;
        if (l_shared < 24) throw std::runtime_error(short_file);
        shared.resize(l_shared);
        if (fread(&shared[0], 1, l_shared, in[0]) != l_shared) throw std::runtime_error(short_file);
        for (size_t gi = 0; gi < in.size(); ++gi) {
            uint32_t l_row;
            if (fread(&l_row, 4, 1, in[gi]) != 1) throw std::runtime_error(short_file);
            rows[gi].resize(l_row);
            if (l_row && fread(rows[gi].data(), 1, l_row, in[gi]) != l_row) throw std::runtime_error(short_file);
            row_of[gi] = {rows[gi].data(), l_row};
        }
        const uint32_t nfs = n_fmt << 24 | n_samples;
        memcpy(&shared[20], &nfs, 4);
        if (counts) {
            uint32_t A, ns;
            ac.clear();
            if (!counts->next(A, ns, ac)) throw std::runtime_error(counts->short_file);
            bcf_put_info(shared, 0, hdr, ac.data(), A, ns);
        }
        indiv.clear();
        bcf_paste_rows(row_of, planes, n_fmt, indiv);
        bcf_put_u32(out, (uint32_t)shared.size());
        bcf_put_u32(out, (uint32_t)indiv.size());
        out += shared;
        out += indiv;
        if (out.size() >= (1u << 20)) flush();
    }
    flush();
    if (bgzf) sink(bgzf_eof().data(), bgzf_eof().size());
}

} // namespace malva
