// The merged output of `call --cohort --merged` as BCF2 (--merged-format bcf | ubcf): the header and its dictionaries, a record's
// shared block, the paste of the groups' per-sample blocks, and a BGZF writer.  No device in here: a record's per-sample block
// comes from mg_encode_calls_bcf, everything around it is made from what the text path has (Rec::prefix, the allele count, the
// site counts).  Written from the published VCF/BCF specification (v4.3, section 6), as the reader in io.hpp is: no file written
// by htslib / bcftools was available, parity UNPINNED; tests/bcf_writer.py and the decoder of tests/test_bcf_out_cpu.py are the
// independent readings the tests use.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace malva {

// ---- typed values (section 6.3.3) ------------------------------------------------------------------------------------------------
// smallest of int8 (1), int16 (2), int32 (3) that holds [lo, hi] with the reserved codes (missing, end of vector) kept free
inline int bcf_int_type(int64_t lo, int64_t hi)
{
    if (lo >= -120 && hi <= 127) return 1;
    if (lo >= -32760 && hi <= 32767) return 2;
    return 3;
}
inline size_t bcf_width(int t) { return t == 3 ? 4 : (size_t)t; }
inline void bcf_put_int(std::string &out, int32_t v, int t) // little endian
{
    for (size_t b = 0; b < bcf_width(t); ++b) out += (char)((uint32_t)v >> (8 * b));
}
inline void bcf_put_u32(std::string &out, uint32_t v) { out.append((const char *)&v, 4); } // (the hosts this builds for are little endian)
inline void bcf_put_typed_int(std::string &out, int32_t v)
{
    const int t = bcf_int_type(v, v);
    out += (char)(0x10 | t);
    bcf_put_int(out, v, t);
}
inline void bcf_put_desc(std::string &out, size_t n, int t)
{
    if (n < 15) {
        out += (char)(n << 4 | (size_t)t);
        return;
    }
    out += (char)(0xF0 | t);
    bcf_put_typed_int(out, (int32_t)n);
}
inline void bcf_put_typed_str(std::string &out, const char *s, size_t n)
{
    bcf_put_desc(out, n, 7);
    out.append(s, n);
}

// ---- the header ------------------------------------------------------------------------------------------------------------------
// The dictionaries of a header text (section 6.2.1), as LineReader::bcf_open and tests/bcf_writer.py restate them: PASS is 0, every
// other FILTER / INFO / FORMAT ID is numbered in order of first appearance, twice the same ID is one entry, an explicit IDX= is
// honoured; the contigs have a dictionary of their own.
struct BcfHeader {
    std::string text;                  // the header lines, '\n' behind each, #CHROM line last
    std::map<std::string, int32_t> ids, contigs;
    bool declared_contigs = false;     // the panel's header had ##contig lines (else they were added from the reference)
    int32_t key(const std::string &id) const
    {
        auto it = ids.find(id);
        if (it == ids.end()) throw std::runtime_error("BCF: the header declares no " + id);
        return it->second;
    }
    int32_t contig(const std::string &name) const
    {
        auto it = contigs.find(name);
        if (it == contigs.end()) throw std::runtime_error("BCF: contig " + name + " is in none of the header's ##contig lines");
        return it->second;
    }
    std::string file_head() const // magic, l_text, the NUL-terminated text
    {
        std::string out("BCF\2\2", 5);
        bcf_put_u32(out, (uint32_t)text.size() + 1);
        out += text;
        out += '\0';
        return out;
    }
};

inline std::string bcf_header_attr(const std::string &line, const char *key) // value of key= inside <...>, unquoted
{
    const std::string k = std::string(key) + "=";
    size_t at = line.find('<');
    while (at != std::string::npos) {
        at = line.find(k, at);
        if (at == std::string::npos) break;
        if (line[at - 1] == '<' || line[at - 1] == ',') {
            size_t b = at + k.size(), e = b;
            if (b < line.size() && line[b] == '"') e = line.find('"', ++b);
            else
                while (e < line.size() && line[e] != ',' && line[e] != '>') ++e;
            return line.substr(b, e == std::string::npos ? std::string::npos : e - b);
        }
        ++at;
    }
    return std::string();
}

inline bool bcf_has_contig_lines(const std::vector<std::string> &lines)
{
    for (const auto &l : lines)
        if (l.rfind("##contig=", 0) == 0) return true;
    return false;
}

// the ##contig lines a header without any gets: one per reference sequence, in FASTA order
inline std::vector<std::string> bcf_contig_lines(const std::vector<std::string> &names, const std::map<std::string, std::string> &seqs)
{
    std::vector<std::string> out;
    for (const auto &n : names) out.push_back("##contig=<ID=" + n + ",length=" + std::to_string(seqs.at(n).size()) + ">");
    return out;
}

inline BcfHeader bcf_parse_header(const std::string &text, bool declared_contigs)
{
    BcfHeader h;
    h.text = text;
    h.declared_contigs = declared_contigs;
    std::vector<std::string> dict{"PASS"}, contigs;
    auto put = [](std::vector<std::string> &d, const std::string &id, const std::string &idx, size_t next) {
        const size_t at = idx.empty() ? next : (size_t)strtoul(idx.c_str(), nullptr, 10);
        if (d.size() <= at) d.resize(at + 1);
        d[at] = id;
    };
    size_t next_contig = 0;
    for (size_t a = 0; a < text.size();) {
        size_t b = text.find('\n', a);
        if (b == std::string::npos) b = text.size();
        const std::string line = text.substr(a, b - a);
        a = b + 1;
        if (line.rfind("##INFO=", 0) == 0 || line.rfind("##FORMAT=", 0) == 0 || line.rfind("##FILTER=", 0) == 0) {
            const std::string id = bcf_header_attr(line, "ID"), idx = bcf_header_attr(line, "IDX");
            bool have = id == "PASS";
            for (const auto &d : dict) have = have || d == id;
            if (have && idx.empty()) continue;
            put(dict, id, idx, dict.size());
        } else if (line.rfind("##contig=", 0) == 0) {
            put(contigs, bcf_header_attr(line, "ID"), bcf_header_attr(line, "IDX"), next_contig);
            next_contig = contigs.size();
        }
    }
    for (size_t i = dict.size(); i-- > 0;) // (the first entry of an ID is the one its key names)
        if (!dict[i].empty()) h.ids[dict[i]] = (int32_t)i;
    for (size_t i = contigs.size(); i-- > 0;)
        if (!contigs[i].empty()) h.contigs[contigs[i]] = (int32_t)i;
    return h;
}

// ---- a record ----------------------------------------------------------------------------------------------------------------------
// The shared block of the record whose first six VCF columns are `prefix` (CHROM POS ID REF ALT QUAL, tab-separated: Rec::prefix),
// FILTER = PASS, no INFO yet (bcf_put_info appends it), n_fmt fields of n_sample samples.
inline void bcf_put_shared(std::string &out, const BcfHeader &h, const std::string &prefix, uint32_t n_fmt, uint32_t n_sample)
{
    size_t col[7];
    col[0] = 0;
    for (int i = 1; i < 6; ++i) {
        const size_t t = prefix.find('\t', col[i - 1]);
        if (t == std::string::npos) throw std::runtime_error("internal: a record's fixed columns are short");
        col[i] = t + 1;
    }
    col[6] = prefix.size() + 1;
    auto len = [&](int i) { return col[i + 1] - 1 - col[i]; };
    const char *p = prefix.data();
    const int32_t chrom = h.contig(prefix.substr(0, len(0)));
    const int32_t pos0 = (int32_t)(strtol(p + col[1], nullptr, 10) - 1), rlen = (int32_t)len(3);
    uint32_t qual = 0x7F800001u; // the missing float
    if (!(len(5) == 1 && p[col[5]] == '.')) {
        const float q = strtof(p + col[5], nullptr);
        memcpy(&qual, &q, 4);
    }
    uint32_t n_allele = 1;
    if (!(len(4) == 1 && p[col[4]] == '.')) {
        ++n_allele;
        for (size_t i = col[4]; i < col[5] - 1; ++i) n_allele += p[i] == ',';
    }
    bcf_put_u32(out, (uint32_t)chrom);
    bcf_put_u32(out, (uint32_t)pos0);
    bcf_put_u32(out, (uint32_t)rlen);
    bcf_put_u32(out, qual);
    bcf_put_u32(out, n_allele << 16); // (n_info: bcf_put_info)
    bcf_put_u32(out, n_fmt << 24 | n_sample);
    if (len(2) == 1 && p[col[2]] == '.') bcf_put_typed_str(out, p, 0);
    else bcf_put_typed_str(out, p + col[2], len(2));
    bcf_put_typed_str(out, p + col[3], len(3));
    for (size_t a = col[4]; n_allele > 1 && a < col[5];) {
        size_t e = a;
        while (e < col[5] - 1 && p[e] != ',') ++e;
        bcf_put_typed_str(out, p + a, e - a);
        a = e + 1;
    }
    out += (char)0x11; // FILTER: the vector [0] = PASS
    out += (char)0;
}

// AF of `ac` copies among `an` as DESIGN.md section 8 rounds it: q millionths, half up
inline uint32_t bcf_af_q(uint32_t ac, uint64_t an) { return (uint32_t)((2ull * ac * 1000000ull + an) / (2ull * an)); }

// --site-tags: INFO of a record from its counts (ac[0 .. A): the called copies per allele, REF first; ns: the called samples),
// appended to the shared block that starts at out[shared_at] -- AC (int vector), AN (int), AF (float vector: (float)(q / 1e6), the
// missing float when AN is 0), NS (int); a record without ALT: AN and NS alone
inline void bcf_put_info(std::string &out, size_t shared_at, const BcfHeader &h, const uint32_t *ac, uint32_t A, uint32_t ns)
{
    uint64_t an = 0;
    for (uint32_t a = 0; a < A; ++a) an += ac[a];
    uint32_t n_info = 2;
    if (A > 1) {
        n_info = 4;
        int64_t lo = ac[1], hi = ac[1];
        for (uint32_t a = 2; a < A; ++a) {
            lo = std::min<int64_t>(lo, ac[a]);
            hi = std::max<int64_t>(hi, ac[a]);
        }
        const int t = bcf_int_type(lo, hi);
        bcf_put_typed_int(out, h.key("AC"));
        bcf_put_desc(out, A - 1, t);
        for (uint32_t a = 1; a < A; ++a) bcf_put_int(out, (int32_t)ac[a], t);
    }
    bcf_put_typed_int(out, h.key("AN"));
    bcf_put_typed_int(out, (int32_t)an);
    if (A > 1) {
        bcf_put_typed_int(out, h.key("AF"));
        bcf_put_desc(out, A - 1, 5);
        for (uint32_t a = 1; a < A; ++a) {
            uint32_t bits = 0x7F800001u;
            if (an) {
                const float f = (float)((double)bcf_af_q(ac[a], an) / 1e6);
                memcpy(&bits, &f, 4);
            }
            bcf_put_u32(out, bits);
        }
    }
    bcf_put_typed_int(out, h.key("NS"));
    bcf_put_typed_int(out, (int32_t)ns);
    uint32_t nai;
    memcpy(&nai, &out[shared_at + 16], 4);
    nai = (nai & 0xFFFF0000u) | n_info;
    memcpy(&out[shared_at + 16], &nai, 4);
}

// ---- the paste of the groups' per-sample blocks ------------------------------------------------------------------------------------
// rows[g]: group g's block of one record (planes[g] samples, n_fmt fields, each at the type the group chose).  The cohort's block
// is appended to `out`: per field the key, the descriptor at the widest of the groups' types -- the smallest type that holds the
// values of all of them -- and the groups' values one behind the other, sign-extended where a group was narrower (GT's missing
// code 0 and every other value keep their meaning).  GT, GQ and COVS never hold a reserved code of their own type; PL of --pl does --
// the missing code and the end-of-vector code of a narrower group's int8 or int16 become those of the wider type (no VALUE of such a
// group equals either: its type was chosen to keep them free).  A float field (GP of --gp) has one type: nothing to widen, the groups'
// values are joined as they are.
inline void bcf_paste_rows(const std::vector<std::pair<const unsigned char *, size_t>> &rows, const std::vector<uint32_t> &planes, uint32_t n_fmt, std::string &out)
{
    struct Cur {
        const unsigned char *p, *e;
        void need(size_t n) const
        {
            if ((size_t)(e - p) < n) throw std::runtime_error("internal: a group's block of the merged output overruns its length");
        }
        int32_t int_of(int t)
        {
            need(bcf_width(t));
            int32_t v;
            if (t == 1) v = (int8_t)p[0];
            else if (t == 2) {
                int16_t w;
                memcpy(&w, p, 2);
                v = w;
            } else
                memcpy(&v, p, 4);
            p += bcf_width(t);
            return v;
        }
        void desc(int &t, uint32_t &n, bool or_float = false)
        {
            need(1);
            const uint32_t d = *p++;
            t = (int)(d & 15);
            n = d >> 4;
            if ((t < 1 || t > 3) && !(or_float && t == 5)) throw std::runtime_error("internal: a group's block of the merged output holds a type that is no integer");
            if (n == 15) {
                int t2;
                uint32_t one;
                desc(t2, one);
                n = (uint32_t)int_of(t2);
            }
        }
    };
    std::vector<Cur> cur;
    for (const auto &r : rows) cur.push_back({r.first, r.first + r.second});
    std::vector<int> ts(rows.size());
    for (uint32_t f = 0; f < n_fmt; ++f) {
        int32_t key = 0;
        uint32_t n = 0;
        int T = 1;
        for (size_t g = 0; g < cur.size(); ++g) {
            int t1;
            uint32_t one, n_g;
            cur[g].desc(t1, one);
            const int32_t key_g = cur[g].int_of(t1);
            cur[g].desc(ts[g], n_g, true);
            if (g && (key_g != key || n_g != n || (ts[g] == 5) != (T == 5))) throw std::runtime_error("internal: the groups' blocks of the merged output disagree");
            key = key_g;
            n = n_g;
            T = std::max(T, ts[g]);
        }
        bcf_put_typed_int(out, key);
        bcf_put_desc(out, n, T);
        for (size_t g = 0; g < cur.size(); ++g) {
            const size_t bytes = (size_t)planes[g] * n * (T == 5 ? 4 : bcf_width(ts[g]));
            cur[g].need(bytes);
            if (ts[g] == T) {
                out.append((const char *)cur[g].p, bytes);
                cur[g].p += bytes;
            } else
                for (size_t i = 0; i < (size_t)planes[g] * n; ++i) {
                    const int32_t v = cur[g].int_of(ts[g]), missing_g = ts[g] == 1 ? INT8_MIN : INT16_MIN, missing_T = T == 2 ? INT16_MIN : INT32_MIN;
                    bcf_put_int(out, v == missing_g ? missing_T : v == missing_g + 1 ? missing_T + 1 : v, T);
                }
        }
    }
    for (const auto &c : cur)
        if (c.p != c.e) throw std::runtime_error("internal: a group's block of the merged output is longer than its fields");
}

// ---- BGZF ------------------------------------------------------------------------------------------------------------------------
// `n` bytes as whole BGZF members appended to `out`: at most 0xFF00 input bytes each, deflated raw at level 6, with the BC extra field
// (BSIZE = member size - 1), CRC32 and ISIZE.  A member boundary may fall anywhere in the stream, so whoever holds a piece of the
// file compresses it alone.
inline void bgzf_append(const char *data, size_t n, std::string &out)
{
    static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    unsigned char body[0x10000];
    for (size_t at = 0; at < n;) {
        const size_t take = std::min<size_t>(n - at, 0xFF00);
        z_stream zs{};
        if (deflateInit2(&zs, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("BGZF: deflateInit2 failed");
        zs.next_in = (Bytef *)(data + at);
        zs.avail_in = (uInt)take;
        zs.next_out = body;
        zs.avail_out = (uInt)(0x10000 - 18 - 8);
        const int rc = deflate(&zs, Z_FINISH);
        const size_t clen = (size_t)zs.total_out;
        deflateEnd(&zs);
        if (rc != Z_STREAM_END) throw std::runtime_error("BGZF: a block does not fit a member");
        const uint32_t bsize = (uint32_t)(18 + clen + 8 - 1), crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(data + at), (uInt)take);
        out.append((const char *)head, 16);
        out += (char)(bsize & 0xFF);
        out += (char)(bsize >> 8);
        out.append((const char *)body, clen);
        bcf_put_u32(out, crc);
        bcf_put_u32(out, (uint32_t)take);
        at += take;
    }
}
// the empty member that ends a BGZF file
inline std::string bgzf_eof()
{
    static const unsigned char eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return std::string((const char *)eof, 28);
}

} // namespace malva
