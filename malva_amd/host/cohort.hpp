// cohort.hpp -- the manifest of `malva-geno call --cohort`: one sample per line, NAME<TAB>INPUT; '#' lines and blank lines are
// skipped.  INPUT is anything the third argument of `call` takes, resolved in the same order (a KMC database at the prefix,
// <prefix>.txt, @list / a comma list of reads, a reads file, a text dump); a relative path is relative to the manifest.  The
// reference has no counterpart: it runs one call_main (main.cpp:421-594) per individual.  Everything here runs before any
// device is created; every error names the manifest and the line.
#pragma once
#include <sys/stat.h>
#include <fstream>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "kmc_db.hpp"
#include "reads.hpp"

namespace malva {

struct SampleInput {
    enum Kind { KMC_DB, TABLE, READS } kind = TABLE;
    std::string path;               // the database prefix or the text table
    std::vector<std::string> reads; // READS: the files
};
struct CohortSample {
    std::string name;
    SampleInput input;
};

inline bool cohort_file_exists(const std::string &p) // (a regular file, as `call` has always asked of its third argument)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
// the detection order of `call`'s third argument; throws std::runtime_error("ERROR: ...") on an input that cannot be read
inline SampleInput resolve_sample_input(const std::string &arg, unsigned ref_k, unsigned max_packed_k)
{
    SampleInput in;
    in.path = arg;
    if (KmcDb::present(arg)) {
        in.kind = SampleInput::KMC_DB;
        return in;
    }
    if (cohort_file_exists(arg + ".txt")) {
        in.path = arg + ".txt";
        return in;
    }
    if (reads_input(arg, &in.reads)) {
        if (ref_k > max_packed_k)
            throw std::runtime_error("ERROR: counting reads needs -r <= " + std::to_string(max_packed_k) + " (the packed k-mer paths; -r " + std::to_string(ref_k) +
                                     "): give a k-mer table instead");
        reads_check_heads(in.reads); // (before any device: a file that is not reads fails at once)
        in.kind = SampleInput::READS;
        return in;
    }
    if (!cohort_file_exists(arg)) throw std::runtime_error("ERROR: cannot open " + arg);
    return in;
}

inline std::vector<CohortSample> read_cohort_manifest(const std::string &path, unsigned ref_k, unsigned max_packed_k)
{
    std::ifstream f(path.c_str());
    if (!f.good()) throw std::runtime_error("ERROR: cannot open the cohort manifest " + path);
    const size_t slash = path.find_last_of('/');
    const std::string dir = slash == std::string::npos ? std::string() : path.substr(0, slash + 1);
    std::vector<CohortSample> out;
    std::set<std::string> seen;
    std::string line;
    size_t no = 0;
    auto bad = [&](const std::string &what) { return std::runtime_error("ERROR: " + path + ":" + std::to_string(no) + ": " + what); };
    while (std::getline(f, line)) {
        ++no;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '#' || line.find_first_not_of(" \t") == std::string::npos) continue;
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) throw bad("no tab: a line is NAME<TAB>INPUT");
        CohortSample s;
        s.name = line.substr(0, tab);
        std::string input = line.substr(tab + 1);
        if (s.name.empty()) throw bad("empty sample name");
        if (s.name.find('/') != std::string::npos) throw bad("sample name '" + s.name + "' contains '/'");
        if (!seen.insert(s.name).second) throw bad("sample name '" + s.name + "' is listed twice");
        if (input.empty()) throw bad("empty input");
        // relative paths are relative to the manifest (each member of a comma list; an @list file itself)
        auto rel = [&](const std::string &p) { return p.empty() || p[0] == '/' || dir.empty() ? p : dir + p; };
        if (input[0] == '@') input = "@" + rel(input.substr(1));
        else if (input.find(',') != std::string::npos) {
            std::string joined;
            size_t a = 0;
            while (a <= input.size()) {
                const size_t c = input.find(',', a);
                const std::string piece = input.substr(a, c == std::string::npos ? std::string::npos : c - a);
                joined += (joined.empty() ? "" : ",") + rel(piece);
                if (c == std::string::npos) break;
                a = c + 1;
            }
            input = joined;
        } else input = rel(input);
        try {
            s.input = resolve_sample_input(input, ref_k, max_packed_k);
        } catch (const std::exception &e) {
            std::string m = e.what();
            if (m.compare(0, 7, "ERROR: ") == 0) m = m.substr(7);
            throw bad("sample '" + s.name + "': " + m);
        }
        out.push_back(std::move(s));
    }
    if (out.empty()) throw std::runtime_error("ERROR: " + path + ": no samples");
    return out;
}

} // namespace malva
