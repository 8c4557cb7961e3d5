// pca.hpp -- the host side of `malva-geno pca`: its command line (a parser and a usage text of its own; USAGE and OPTIONS of index / call
// do not know the sub-command), the two readers of a genetic relationship matrix as `call --cohort --grm` writes it, and the three output
// files.  Nothing here touches the device: main.cpp's pca_main hands the matrix to mg_pca_load_* / mg_pca_solve, and
// tools/pca_host_check.cpp runs everything in this file without one.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <ostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "part_file.hpp"

namespace malva {

constexpr uint32_t PCA_MAX_N = 16384, PCA_MAX_K = 32; // MG_PCA_MAX_N, MG_PCA_MAX_K

inline const char *const PCA_USAGE =
    "Usage: malva-geno pca [--pcs K] [--tol T] [--max-iters N] [-d DEVICE] -o OUT <GRM>\n"
    "\n"
    "Principal components of a genetic relationship matrix, solved on the GPU (blocked subspace\n"
    "iteration with Rayleigh-Ritz, in double; include/malva_hip.h, mg_pca_solve).\n"
    "\n"
    "Arguments:\n"
    "      <GRM>                             what `call --cohort --grm` wrote: with <GRM>.grm.bin present, that\n"
    "                                        file and <GRM>.grm.id (--grm-format gcta); else <GRM> is the text table\n"
    "      -o, --out OUT                     writes OUT.eigenval, OUT.eigenvec (NAME NAME PC1 .. PCK, as GCTA and\n"
    "                                        PLINK do) and OUT.pca.tsv (PC EIGENVALUE SHARE RESIDUAL CONVERGED)\n"
    "      --pcs K                           components, 1..32 (default:20, as in GCTA and PLINK); lowered to the\n"
    "                                        number of samples where that is smaller\n"
    "      --tol T                           a component is converged when ||G v - theta v|| <= T max|theta|;\n"
    "                                        0 < T < 1 (default:1e-10 -- a design choice, not a measurement)\n"
    "      --max-iters N                     products G Q at most, 1..1000000 (default:2000)\n"
    "      -d, --device DEVICE               GPU to run on (default:0)\n"
    "      -h, --help                        this text\n"
    "\n"
    "Exit status: 0 when all K components converged; 2 when some did not (all three files are written\n"
    "and stderr names the first one); 1 for a refused command line or input, with nothing written.\n";

struct PcaOptions {
    uint32_t pcs = 20, max_iters = 2000;
    double tol = 1e-10;
    int device = 0;
    std::string out, grm;
};
enum class PcaParsed { ok, help, refused };

inline bool pca_whole_number(const char *text, uint64_t lo, uint64_t hi, uint64_t *out)
{
    if (!*text || strlen(text) > 12) return false;
    uint64_t v = 0;
    for (const char *p = text; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        v = 10 * v + (uint64_t)(*p - '0');
    }
    *out = v;
    return v >= lo && v <= hi;
}

// argv[0] is "pca".  One `malva : ...` line per fault and PCA_USAGE go to err when the line is refused
inline PcaParsed pca_parse(int argc, const char *const *argv, PcaOptions &o, std::ostream &err)
{
    struct Row {
        const char *name;
        char letter;
        bool arg;
    };
    static const Row rows[] = {{"pcs", 0, true}, {"tol", 0, true}, {"max-iters", 0, true}, {"device", 'd', true}, {"out", 'o', true}, {"help", 'h', false}};
    int faults = 0;
    bool help = false;
    std::vector<std::string> rest;
    auto fault = [&](const std::string &what) {
        err << "malva : " << what << "\n";
        ++faults;
    };
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a.size() < 2 || a[0] != '-') {
            rest.push_back(a);
            continue;
        }
        const Row *row = nullptr;
        std::string value;
        bool attached = false;
        if (a[1] == '-') {
            const size_t eq = a.find('=');
            const std::string name = a.substr(2, eq == std::string::npos ? std::string::npos : eq - 2);
            for (const Row &r : rows)
                if (name == r.name) row = &r;
            if (eq != std::string::npos) value = a.substr(eq + 1), attached = true;
        } else {
            for (const Row &r : rows)
                if (r.letter && a[1] == r.letter) row = &r;
            if (a.size() > 2) value = a.substr(2), attached = true;
        }
        if (!row) {
            fault("unknown option " + a);
            continue;
        }
        if (!row->arg) {
            if (attached) fault("option --" + std::string(row->name) + " takes no value");
            else help = true;
            continue;
        }
        if (!attached) {
            if (i + 1 >= argc) {
                fault("option --" + std::string(row->name) + " needs a value");
                continue;
            }
            value = argv[++i];
        }
        const std::string name = row->name;
        uint64_t v = 0;
        if (name == "pcs") {
            if (pca_whole_number(value.c_str(), 1, PCA_MAX_K, &v)) o.pcs = (uint32_t)v;
            else fault("--pcs takes 1..32");
        } else if (name == "max-iters") {
            if (pca_whole_number(value.c_str(), 1, 1000000, &v)) o.max_iters = (uint32_t)v;
            else fault("--max-iters takes 1..1000000");
        } else if (name == "device") {
            if (pca_whole_number(value.c_str(), 0, 1023, &v)) o.device = (int)v;
            else fault("--device takes a device number");
        } else if (name == "tol") {
            char *end = nullptr;
            errno = 0;
            const double t = value.empty() ? 0.0 : strtod(value.c_str(), &end);
            if (value.empty() || *end || errno || !std::isfinite(t) || !(t > 0.0 && t < 1.0) || value.find_first_of("xXnNiI \t") != std::string::npos) fault("--tol takes a number above 0 and below 1");
            else o.tol = t;
        } else o.out = value;
    }
    if (help) return PcaParsed::help;
    if (o.out.empty()) fault("pca needs -o OUT");
    if (rest.size() != 1) fault(rest.empty() ? "pca needs one <GRM>" : "pca takes one <GRM>, not " + std::to_string(rest.size()));
    else if (rest[0].empty()) fault("<GRM> is empty");
    else o.grm = rest[0];
    if (faults) {
        err << PCA_USAGE;
        return PcaParsed::refused;
    }
    return PcaParsed::ok;
}

// A matrix as read: the names in input order and either GCTA's float triangle (row by row, diagonal included) or the lower triangle of a
// full double array, [n][n] row-major, whose upper triangle is left 0 and is never read.  trace: the diagonal summed in order, in double
struct PcaInput {
    std::vector<std::string> names;
    bool packed = false;
    std::vector<float> tri;
    std::vector<double> full;
    double trace = 0.0;
};

inline bool pca_file_exists(const std::string &path)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

// PREFIX.grm.id (FID<tab>IID per sample; the sample's name is the IID) and PREFIX.grm.bin
inline PcaInput pca_read_gcta(const std::string &prefix)
{
    PcaInput in;
    in.packed = true;
    const std::string id_path = prefix + ".grm.id", bin_path = prefix + ".grm.bin";
    std::ifstream ids(id_path);
    if (!ids) throw std::runtime_error("cannot read " + id_path);
    std::string line;
    size_t line_no = 0;
    while (std::getline(ids, line)) {
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        const size_t tab = line.rfind('\t');
        const std::string name = tab == std::string::npos ? line : line.substr(tab + 1);
        if (name.empty()) throw std::runtime_error(id_path + " line " + std::to_string(line_no) + ": no sample name");
        in.names.push_back(name);
        if (in.names.size() > PCA_MAX_N) throw std::runtime_error(id_path + ": more than " + std::to_string(PCA_MAX_N) + " samples");
    }
    const size_t n = in.names.size();
    if (!n) throw std::runtime_error(id_path + " names no sample");
    FILE *f = fopen(bin_path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + bin_path);
    const size_t want = n * (n + 1) / 2;
    in.tri.resize(want);
    const size_t got = fread(in.tri.data(), 4, want, f);
    char extra;
    const bool more = got == want && fread(&extra, 1, 1, f) == 1;
    fclose(f);
    if (got != want || more)
        throw std::runtime_error(bin_path + " does not hold the " + std::to_string(want) + " floats (n (n + 1) / 2) of the " + std::to_string(n) + " samples of " + id_path);
    for (size_t i = 0; i < n; ++i) in.trace += (double)in.tri[i * (i + 1) / 2 + i];
    return in;
}

// the text table of --grm: a header line, then NAME_A<tab>NAME_B<tab>N<tab>GRM, one line per pair; the names are those of the A == B
// lines, in order; `.` is 0
inline PcaInput pca_read_table(const std::string &path)
{
    struct Line {
        std::string a, b, value;
        size_t no;
    };
    std::ifstream f(path);
    if (!f) throw std::runtime_error("cannot read " + path);
    std::vector<Line> lines;
    std::string text;
    size_t no = 0;
    PcaInput in;
    std::unordered_map<std::string, uint32_t> index;
    auto at = [&](size_t k) { return path + " line " + std::to_string(k) + ": "; };
    while (std::getline(f, text)) {
        ++no;
        if (!text.empty() && text.back() == '\r') text.pop_back();
        if (text.empty() || (no == 1 && text[0] == '#')) continue;
        Line l;
        l.no = no;
        const size_t t1 = text.find('\t'), t2 = t1 == std::string::npos ? t1 : text.find('\t', t1 + 1), t3 = t2 == std::string::npos ? t2 : text.find('\t', t2 + 1);
        if (t3 == std::string::npos || text.find('\t', t3 + 1) != std::string::npos) throw std::runtime_error(at(no) + "not the four columns A B N GRM");
        l.a = text.substr(0, t1), l.b = text.substr(t1 + 1, t2 - t1 - 1), l.value = text.substr(t3 + 1);
        if (l.a == l.b) {
            if (!index.emplace(l.a, (uint32_t)in.names.size()).second) throw std::runtime_error(at(no) + "the pair " + l.a + " " + l.b + " is given twice");
            in.names.push_back(l.a);
            if (in.names.size() > PCA_MAX_N) throw std::runtime_error(path + ": more than " + std::to_string(PCA_MAX_N) + " samples");
        }
        lines.push_back(std::move(l));
    }
    const size_t n = in.names.size();
    if (!n) throw std::runtime_error(path + " holds no sample (no line with A == B)");
    in.full.assign(n * n, 0.0);
    std::vector<bool> seen(n * n, false);
    for (const Line &l : lines) {
        const auto ia = index.find(l.a), ib = index.find(l.b);
        if (ia == index.end() || ib == index.end()) throw std::runtime_error(at(l.no) + "unknown name " + (ia == index.end() ? l.a : l.b) + " (no line pairs it with itself)");
        const size_t hi = ia->second > ib->second ? ia->second : ib->second, lo = ia->second > ib->second ? ib->second : ia->second;
        if (seen[hi * n + lo] && hi != lo) throw std::runtime_error(at(l.no) + "the pair " + l.a + " " + l.b + " is given twice");
        seen[hi * n + lo] = true;
        double v = 0.0;
        if (l.value != ".") {
            char *end = nullptr;
            errno = 0;
            v = l.value.empty() ? 0.0 : strtod(l.value.c_str(), &end);
            if (l.value.empty() || *end || errno || !std::isfinite(v) || l.value.find_first_of("xX \t") != std::string::npos) throw std::runtime_error(at(l.no) + "cannot read the number " + l.value);
        }
        in.full[hi * n + lo] = v;
    }
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j <= i; ++j)
            if (!seen[i * n + j]) throw std::runtime_error(path + ": the pair " + in.names[j] + " " + in.names[i] + " is missing");
    for (size_t i = 0; i < n; ++i) in.trace += in.full[i * n + i];
    return in;
}

inline PcaInput pca_read(const std::string &grm) { return pca_file_exists(grm + ".grm.bin") ? pca_read_gcta(grm) : pca_read_table(grm); }

// mg_pca_solve's outputs for k components of n samples, and mg_pca_stats'
struct PcaResult {
    uint32_t n = 0, k = 0;
    std::vector<double> values, vectors, resid; // [k], [k][n], [k]
    double scale = 1.0, tol = 0.0;
    uint32_t info[3] = {0, 0, 0}; // products, converged, m
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
};

inline std::string pca_eigenval_text(const PcaResult &r)
{
    std::string out;
    char num[64];
    for (uint32_t j = 0; j < r.k; ++j) {
        snprintf(num, sizeof num, "%.10g\n", r.values[j]);
        out += num;
    }
    return out;
}
inline std::string pca_eigenvec_text(const PcaResult &r, const std::vector<std::string> &names)
{
    if (names.size() != r.n || r.vectors.size() != (size_t)r.k * r.n) throw std::logic_error("pca_eigenvec_text: a result that is not the names'");
    std::string out;
    char num[64];
    for (uint32_t i = 0; i < r.n; ++i) {
        out += names[i] + "\t" + names[i];
        for (uint32_t j = 0; j < r.k; ++j) {
            snprintf(num, sizeof num, "\t%.10g", r.vectors[(size_t)j * r.n + i]);
            out += num;
        }
        out += '\n';
    }
    return out;
}
inline std::string pca_table_text(const PcaResult &r, double trace)
{
    std::string out = "PC\tEIGENVALUE\tSHARE\tRESIDUAL\tCONVERGED\n";
    char line[256], share[64];
    for (uint32_t j = 0; j < r.k; ++j) {
        if (trace > 0.0) snprintf(share, sizeof share, "%.6f", r.values[j] / trace);
        else snprintf(share, sizeof share, ".");
        snprintf(line, sizeof line, "%u\t%.10g\t%s\t%.3e\t%d\n", j + 1, r.values[j], share, r.resid[j], r.resid[j] <= r.tol ? 1 : 0);
        out += line;
    }
    snprintf(line, sizeof line, "# n=%u m=%u products=%u tol=%g ms=%.3f,%.3f,%.3f,%.3f (products, orthonormalisation, Rayleigh-Ritz, total)\n", r.n, r.info[2], r.info[0],
             r.tol, r.ms[0], r.ms[1], r.ms[2], r.ms[3]);
    out += line;
    return out;
}
// -> the first component that is not converged, or k
inline uint32_t pca_first_unconverged(const PcaResult &r)
{
    for (uint32_t j = 0; j < r.k; ++j)
        if (!(r.resid[j] <= r.tol)) return j;
    return r.k;
}

// OUT.eigenval, OUT.eigenvec, OUT.pca.tsv: all three written under temporary names, closed, then renamed; a failure leaves none behind
inline void pca_write(const std::string &out, const PcaResult &r, const std::vector<std::string> &names, double trace)
{
    PartFile files[3];
    const std::string text[3] = {pca_eigenval_text(r), pca_eigenvec_text(r, names), pca_table_text(r, trace)};
    const char *suffix[3] = {".eigenval", ".eigenvec", ".pca.tsv"};
    for (int i = 0; i < 3; ++i) files[i].open(out + suffix[i]);
    for (int i = 0; i < 3; ++i) files[i].write(text[i]);
    for (int i = 0; i < 3; ++i) files[i].close();
    try {
        for (int i = 0; i < 3; ++i) files[i].finish();
    } catch (...) {
        for (int i = 0; i < 3; ++i)
            if (files[i].part.empty()) unlink(files[i].path.c_str()); // (already under its name)
        throw;
    }
}

} // namespace malva
