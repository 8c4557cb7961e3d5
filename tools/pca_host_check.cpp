// The host half of `malva-geno pca` (malva_amd/host/pca.hpp, csrc/pca_plan.h) driven without a device: the two readers on files made by
// grm_gcta and grm_text of cohort_out.hpp and on every broken input they must name, the three writers and their PATH.part hand-over, the
// sub-command's parser, the block geometry, and the small dense eigen-solver (cyclic Jacobi) on matrices with known spectra.  Meant to be
// built with -fsanitize=address,undefined and run on the CPU (`make sanitize-host`); tests/test_pca_cases_cpu.py builds it plain.  It
// takes a scratch directory as its argument and exits non-zero on the first wrong answer.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <sys/stat.h>

#include "cohort_out.hpp"
#include "pca.hpp"
#include "../malva_amd/csrc/pca_plan.h"

using namespace malva;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::cerr << __FILE__ << ":" << __LINE__ << ": " #cond "\n";       \
            std::cout << "pca_host_check: FAILED\n";                           \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static bool exists(const std::string &p) { return access(p.c_str(), F_OK) == 0; }
static std::string slurp(const std::string &p)
{
    std::ifstream in(p, std::ios::binary);
    std::stringstream all;
    all << in.rdbuf();
    return all.str();
}
static void put(const std::string &p, const std::string &text)
{
    std::ofstream out(p, std::ios::binary);
    out << text;
}
static std::string error_of(const std::function<void()> &run)
{
    try {
        run();
    } catch (const std::runtime_error &e) {
        return e.what();
    }
    return std::string();
}
static bool has(const std::string &text, const char *piece) { return text.find(piece) != std::string::npos; }

// ---- the parser ------------------------------------------------------------------------------------------------------------------------
struct Line {
    PcaParsed parsed;
    PcaOptions o;
    std::string err;
};
static Line parse(std::vector<const char *> words)
{
    words.insert(words.begin(), "pca");
    Line l;
    std::ostringstream err;
    l.parsed = pca_parse((int)words.size(), words.data(), l.o, err);
    l.err = err.str();
    return l;
}
static size_t count(const std::string &text, const char *piece)
{
    size_t n = 0;
    for (size_t at = text.find(piece); at != std::string::npos; at = text.find(piece, at + 1)) ++n;
    return n;
}
static void check_parser()
{
    Line l = parse({"-o", "out", "grm"});
    CHECK(l.parsed == PcaParsed::ok && l.err.empty() && l.o.pcs == 20 && l.o.tol == 1e-10 && l.o.max_iters == 2000 && l.o.device == 0 && l.o.out == "out" && l.o.grm == "grm");
    l = parse({"grm", "--pcs", "32", "--tol=1e-6", "--max-iters", "1000000", "-d3", "--out", "x"});
    CHECK(l.parsed == PcaParsed::ok && l.o.pcs == 32 && l.o.tol == 1e-6 && l.o.max_iters == 1000000 && l.o.device == 3 && l.o.out == "x" && l.o.grm == "grm");
    l = parse({"--pcs=1", "--max-iters=1", "--device", "0", "-oy", "g"});
    CHECK(l.parsed == PcaParsed::ok && l.o.pcs == 1 && l.o.max_iters == 1 && l.o.out == "y");
    for (const char *flag : {"-h", "--help"}) {
        l = parse({flag});
        CHECK(l.parsed == PcaParsed::help && l.err.empty());
    }
    l = parse({"--pcs", "0", "-h"}); // the message ahead of the help comes first, as in call
    CHECK(l.parsed == PcaParsed::help && l.err == "malva : --pcs takes 1..32\n");
    // one message per fault, then the usage
    const std::vector<std::vector<const char *>> refused = {
        {"-o", "out"}, {"grm"}, {"-o", "out", "a", "b"}, {"-o", "out", "g", "--pcs", "0"}, {"-o", "out", "g", "--pcs", "33"}, {"-o", "out", "g", "--pcs", "5x"},
        {"-o", "out", "g", "--pcs", "-1"}, {"-o", "out", "g", "--pcs", ""}, {"-o", "out", "g", "--tol", "0"}, {"-o", "out", "g", "--tol", "1"}, {"-o", "out", "g", "--tol", "-1e-3"},
        {"-o", "out", "g", "--tol", "nan"}, {"-o", "out", "g", "--tol", "inf"}, {"-o", "out", "g", "--tol", "1e-5x"}, {"-o", "out", "g", "--tol", ""}, {"-o", "out", "g", "--tol", "0x1p-3"},
        {"-o", "out", "g", "--max-iters", "0"}, {"-o", "out", "g", "--max-iters", "1000001"}, {"-o", "out", "g", "--max-iters", "1e3"}, {"-o", "out", "g", "-d", "x"},
        {"-o", "out", "g", "--grm"}, {"-o", "out", "g", "-z"}, {"-o", "out", "g", "--pcs"}, {"-o", "out", "g", "--help=1"}, {"-o", "", "g"}, {"-o", "out", ""}};
    for (const auto &words : refused) {
        l = parse(words);
        CHECK(l.parsed == PcaParsed::refused && count(l.err, "malva : ") == 1 && has(l.err, PCA_USAGE) && l.err.rfind(PCA_USAGE) + strlen(PCA_USAGE) == l.err.size());
    }
    l = parse({"--pcs", "99", "--tol", "2", "--max-iters", "0"}); // five faults, five messages
    CHECK(l.parsed == PcaParsed::refused && count(l.err, "malva : ") == 5 && count(l.err, "Usage: malva-geno pca") == 1);
    CHECK(has(PCA_USAGE, "design choice, not a measurement") && has(PCA_USAGE, "default:20") && has(PCA_USAGE, "default:1e-10") && has(PCA_USAGE, "default:2000"));
}

// ---- the readers -----------------------------------------------------------------------------------------------------------------------
static GrmState state_of(size_t S)
{
    GrmState st;
    st.sum.resize(S * (S + 1) / 2), st.n.resize(S * (S + 1) / 2);
    for (size_t a = 0, k = 0; a < S; ++a)
        for (size_t b = a; b < S; ++b, ++k) {
            st.n[k] = 1000 + 7 * a + b;
            st.sum[k] = ((int64_t)(a == b ? 1100000 + 9000 * (int64_t)a : 31000 * (int64_t)((a * 5 + b * 3) % 11) - 150000)) * (int64_t)st.n[k];
        }
    st.n[3] = 0; // a pair without records: `.` in the text, 0 in GCTA's form
    st.sum[3] = 0;
    return st;
}
static void check_readers(const std::string &dir)
{
    const std::vector<std::string> names = {"alpha", "b", "sample three", "d4", "e"};
    const size_t S = names.size();
    const GrmState st = state_of(S);
    // GCTA's three files, as call --grm-format gcta writes them
    const std::string prefix = dir + "/pca_in";
    std::string values, counts, ids;
    grm_gcta(st, names, [&](const char *d, size_t n) { values.append(d, n); }, [&](const char *d, size_t n) { counts.append(d, n); }, [&](const char *d, size_t n) { ids.append(d, n); });
    put(prefix + ".grm.bin", values), put(prefix + ".grm.N.bin", counts), put(prefix + ".grm.id", ids);
    PcaInput in = pca_read(prefix);
    CHECK(in.packed && in.names == names && in.tri.size() == S * (S + 1) / 2 && in.full.empty());
    CHECK(values.size() == 4 * in.tri.size() && !memcmp(values.data(), in.tri.data(), values.size()));
    double trace = 0.0;
    for (size_t i = 0; i < S; ++i) trace += (double)in.tri[i * (i + 1) / 2 + i];
    CHECK(in.trace == trace && trace > 5.0);
    // the text table of the same state
    const std::string table = dir + "/pca_in.tsv";
    std::string text;
    grm_text(st, names, [&](const char *d, size_t n) { text.append(d, n); });
    put(table, text);
    PcaInput tin = pca_read(table);
    CHECK(!tin.packed && tin.names == names && tin.full.size() == S * S && tin.tri.empty());
    for (size_t i = 0; i < S; ++i)
        for (size_t j = 0; j <= i; ++j) {
            const double want = (double)in.tri[i * (i + 1) / 2 + j]; // six decimals of the same value
            CHECK(std::fabs(tin.full[i * S + j] - want) <= 5.7e-7); // (half a unit of the sixth decimal and half a float32 ulp below 2)
            if (j < i) CHECK(tin.full[j * S + i] == 0.0); // the upper triangle is not filled
        }
    CHECK(tin.full[3 * S + 0] == 0.0); // (pair 3 of the state is (0, 3)): `.`
    // pairs in another order and named the other way round read the same
    {
        std::vector<std::string> lines;
        std::istringstream all(text);
        std::string line, head;
        std::getline(all, head);
        while (std::getline(all, line)) lines.push_back(line);
        std::string shuffled = head + "\n";
        for (size_t i = 0; i < lines.size(); ++i) {
            const std::string &l = lines[i];
            const size_t t1 = l.find('\t'), t2 = l.find('\t', t1 + 1);
            shuffled += i % 2 ? l.substr(t1 + 1, t2 - t1 - 1) + "\t" + l.substr(0, t1) + l.substr(t2) + "\n" : l + "\n";
        }
        put(table, shuffled);
        const PcaInput again = pca_read(table);
        CHECK(again.names == names && again.full == tin.full && again.trace == tin.trace);
    }
    // every broken input is named
    put(prefix + ".grm.bin", values.substr(0, values.size() - 4));
    CHECK(has(error_of([&] { pca_read(prefix); }), ".grm.bin does not hold the 15 floats"));
    put(prefix + ".grm.bin", values + "abcd");
    CHECK(has(error_of([&] { pca_read(prefix); }), ".grm.bin does not hold the 15 floats"));
    put(prefix + ".grm.bin", values.substr(0, values.size() - 1));
    CHECK(has(error_of([&] { pca_read(prefix); }), "does not hold"));
    put(prefix + ".grm.bin", values);
    put(prefix + ".grm.id", "");
    CHECK(has(error_of([&] { pca_read(prefix); }), "names no sample"));
    unlink((prefix + ".grm.id").c_str());
    CHECK(has(error_of([&] { pca_read(prefix); }), "cannot read"));
    CHECK(has(error_of([&] { pca_read(dir + "/no_such_table"); }), "cannot read"));
    const std::string head = "#A\tB\tN\tGRM\n";
    struct Bad {
        std::string text;
        const char *line, *what;
    };
    const std::vector<Bad> bad = {
        {head + "a\ta\t5\t1.0\nb\tb\t5\t1.0\n", "", "the pair a b is missing"},
        {head + "a\ta\t5\t1.0\na\tb\t5\t0.1\nb\tb\t5\t1.0\nb\ta\t5\t0.1\n", "line 5: ", "the pair b a is given twice"},
        {head + "a\ta\t5\t1.0\na\ta\t5\t1.0\n", "line 3: ", "the pair a a is given twice"},
        {head + "a\ta\t5\t1.0\na\tc\t5\t0.1\n", "line 3: ", "unknown name c"},
        {head + "a\ta\t5\t1.0x\n", "line 2: ", "cannot read the number 1.0x"},
        {head + "a\ta\t5\tnan\n", "line 2: ", "cannot read the number nan"},
        {head + "a\ta\t5\t\n", "line 2: ", "cannot read the number"},
        {head + "a\ta\t5\n", "line 2: ", "not the four columns"},
        {head + "a\ta\t5\t1.0\t9\n", "line 2: ", "not the four columns"},
        {head, "", "holds no sample"},
    };
    for (const Bad &b : bad) {
        put(table, b.text);
        const std::string e = error_of([&] { pca_read(table); });
        CHECK(has(e, b.what) && has(e, b.line) && has(e, "pca_in.tsv"));
    }
    put(table, head + "a\ta\t0\t.\n");
    CHECK(pca_read(table).full == std::vector<double>{0.0});
}

// ---- the writers -----------------------------------------------------------------------------------------------------------------------
static void check_writers(const std::string &dir)
{
    PcaResult r;
    r.n = 3, r.k = 2, r.tol = 1e-10, r.scale = 2.5;
    r.values = {2.5, -0.125};
    r.vectors = {0.5, -0.25, 1.0 / 3.0, 1e-20, 0.0, -1.0};
    r.resid = {1e-10, 3.25e-7};
    r.info[0] = 12, r.info[1] = 1, r.info[2] = 3;
    r.ms[0] = 1.5f, r.ms[1] = 0.25f, r.ms[2] = 0.125f, r.ms[3] = 2.f;
    const std::vector<std::string> names = {"a", "b b", "c"};
    CHECK(pca_eigenval_text(r) == "2.5\n-0.125\n");
    CHECK(pca_eigenvec_text(r, names) == "a\ta\t0.5\t1e-20\nb b\tb b\t-0.25\t0\nc\tc\t0.3333333333\t-1\n");
    CHECK(pca_table_text(r, 5.0) == "PC\tEIGENVALUE\tSHARE\tRESIDUAL\tCONVERGED\n1\t2.5\t0.500000\t1.000e-10\t1\n2\t-0.125\t-0.025000\t3.250e-07\t0\n"
                                     "# n=3 m=3 products=12 tol=1e-10 ms=1.500,0.250,0.125,2.000 (products, orthonormalisation, Rayleigh-Ritz, total)\n");
    CHECK(has(pca_table_text(r, 0.0), "1\t2.5\t.\t1.000e-10\t1\n") && has(pca_table_text(r, -1.0), "\t.\t"));
    CHECK(pca_first_unconverged(r) == 1);
    r.resid[1] = 0.0;
    CHECK(pca_first_unconverged(r) == 2);
    const std::string out = dir + "/pca_out";
    pca_write(out, r, names, 5.0);
    CHECK(slurp(out + ".eigenval") == pca_eigenval_text(r) && slurp(out + ".eigenvec") == pca_eigenvec_text(r, names) && slurp(out + ".pca.tsv") == pca_table_text(r, 5.0));
    for (const char *s : {".eigenval", ".eigenvec", ".pca.tsv"}) CHECK(!exists(out + s + ".part"));
    // a directory that does not exist: nothing is left, not even the files that opened
    const std::string nowhere = dir + "/no_such_dir/out";
    CHECK(has(error_of([&] { pca_write(nowhere, r, names, 5.0); }), "cannot write"));
    // one of the three names is taken by a directory: the rename fails, and the two that made it are taken back
    const std::string half = dir + "/pca_half";
    mkdir((half + ".pca.tsv").c_str(), 0700);
    put(half + ".pca.tsv/keep", "x");
    CHECK(has(error_of([&] { pca_write(half, r, names, 5.0); }), "cannot write"));
    CHECK(!exists(half + ".eigenval") && !exists(half + ".eigenvec") && !exists(half + ".eigenval.part") && !exists(half + ".eigenvec.part") && !exists(half + ".pca.tsv.part"));
    bool threw = false;
    try {
        pca_eigenvec_text(r, {"a"});
    } catch (const std::logic_error &) {
        threw = true;
    }
    CHECK(threw);
}

// ---- the geometry and the small solver ----------------------------------------------------------------------------------------------------
static void check_plan()
{
    using namespace mg;
    CHECK(pca_block(1, 1) == 1 && pca_block(2, 2) == 2 && pca_block(17, 5) == 17 && pca_block(33, 5) == 32 && pca_block(32, 5) == 32 && pca_block(130, 32) == 64);
    CHECK(pca_block(600, 10) == 32 && pca_block(600, 20) == 48 && pca_block(600, 17) == 48 && pca_block(600, 16) == 32 && pca_block(40, 3) == 32);
    CHECK(pca_np(1) == 16 && pca_np(16) == 16 && pca_np(17) == 32 && pca_np(16384) == 16384);
    for (uint32_t n : {17u, 33u, 257u, 600u, 1024u, 4096u, 5000u, 16384u}) {
        uint32_t chunk = 0;
        const uint32_t np = pca_np(n), splits = pca_splits(np, &chunk);
        CHECK(splits >= 1 && splits <= PCA_MAX_SPLITS && chunk % (PCA_MFMA_K * PCA_WAVES) == 0 && (uint64_t)chunk * splits >= np);
        CHECK(splits == 1 || (uint64_t)chunk * (splits - 1) < np); // no workgroup without work
    }
    uint32_t chunk = 0;
    CHECK(pca_splits(16384, &chunk) == 1 && chunk == 16384);
    CHECK(pca_splits(1024, &chunk) == 4 && chunk == 256);
    CHECK(pca_red_blocks(16) == 1 && pca_red_blocks(256) == 1 && pca_red_blocks(272) == 2);
    // the hash is a function of its three arguments, inside (-1, 1)
    CHECK(pca_hash_value(0, 0, 0) != pca_hash_value(1, 0, 0) && pca_hash_value(0, 0, 0) != pca_hash_value(0, 1, 0) && pca_hash_value(0, 0, 0) != pca_hash_value(0, 0, 1));
    double sum = 0.0;
    for (uint64_t i = 0; i < 4096; ++i) {
        const double h = pca_hash_value(i, 7, 3);
        CHECK(h >= -1.0 && h < 1.0);
        sum += h;
    }
    CHECK(std::fabs(sum / 4096) < 0.05);
}
static void check_jacobi()
{
    using namespace mg;
    // planted spectra: A = V diag(lambda) V^T with V a product of plane rotations
    for (uint32_t n : {1u, 2u, 3u, 16u, 33u, 64u}) {
        std::vector<double> lam(n), V((size_t)n * n, 0.0), A((size_t)n * n, 0.0);
        for (uint32_t i = 0; i < n; ++i) lam[i] = n == 2 ? (i ? -1.0 : 2.0) : i < 2 ? 5.0 : i == 2 ? -20.0 : 3.0 - 0.05 * i; // a double value, a negative one
        for (uint32_t i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
        for (uint32_t p = 0; p + 1 < n; ++p)
            for (uint32_t q = p + 1; q < n; q += 3) {
                const double c = std::cos(0.3 + p + 2 * q), s = std::sin(0.3 + p + 2 * q);
                for (uint32_t i = 0; i < n; ++i) {
                    const double x = V[(size_t)i * n + p], y = V[(size_t)i * n + q];
                    V[(size_t)i * n + p] = c * x - s * y, V[(size_t)i * n + q] = s * x + c * y;
                }
            }
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < n; ++j)
                for (uint32_t t = 0; t < n; ++t) A[(size_t)i * n + j] += V[(size_t)i * n + t] * lam[t] * V[(size_t)j * n + t];
        std::vector<double> a = A, w(n), v((size_t)n * n);
        CHECK(pca_jacobi(n, a.data(), w.data(), v.data()) >= 0);
        std::vector<double> sorted = lam;
        std::sort(sorted.begin(), sorted.end(), std::greater<double>());
        const double L = 20.0, eps = 2.220446049250313e-16;
        for (uint32_t j = 0; j < n; ++j) {
            CHECK(std::fabs(w[j] - sorted[j]) <= 64 * n * eps * L);
            CHECK(j == 0 || w[j] <= w[j - 1]);
            double res = 0.0;
            for (uint32_t i = 0; i < n; ++i) {
                double av = 0.0;
                for (uint32_t t = 0; t < n; ++t) av += 0.5 * (A[(size_t)i * n + t] + A[(size_t)t * n + i]) * v[(size_t)t * n + j];
                res += (av - w[j] * v[(size_t)i * n + j]) * (av - w[j] * v[(size_t)i * n + j]);
            }
            CHECK(std::sqrt(res) <= 64 * n * eps * L);
            for (uint32_t t = 0; t <= j; ++t) {
                double dot = 0.0;
                for (uint32_t i = 0; i < n; ++i) dot += v[(size_t)i * n + j] * v[(size_t)i * n + t];
                CHECK(std::fabs(dot - (t == j ? 1.0 : 0.0)) <= 64 * n * eps);
            }
        }
    }
    // the zero matrix: no sweep, the unit vectors
    std::vector<double> z(9, 0.0), w(3), v(9);
    CHECK(mg::pca_jacobi(3, z.data(), w.data(), v.data()) == 0 && w == std::vector<double>(3, 0.0) && v == std::vector<double>({1, 0, 0, 0, 1, 0, 0, 0, 1}));
    // only the upper triangle is read
    std::vector<double> u = {2.0, 1.0, 1e300, 2.0};
    CHECK(mg::pca_jacobi(2, u.data(), w.data(), v.data()) >= 0 && std::fabs(w[0] - 3.0) < 1e-14 && std::fabs(w[1] - 1.0) < 1e-14);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::cerr << "usage: pca_host_check SCRATCH_DIR\n";
        return 2;
    }
    const std::string dir = argv[1];
    check_parser();
    check_readers(dir);
    check_writers(dir);
    check_plan();
    check_jacobi();
    for (const char *f : {"/pca_in.grm.bin", "/pca_in.grm.N.bin", "/pca_in.grm.id", "/pca_in.tsv", "/pca_out.eigenval", "/pca_out.eigenvec", "/pca_out.pca.tsv", "/pca_half.pca.tsv/keep"})
        unlink((dir + f).c_str());
    rmdir((dir + "/pca_half.pca.tsv").c_str());
    std::cout << "pca_host_check: ok\n";
    return 0;
}
