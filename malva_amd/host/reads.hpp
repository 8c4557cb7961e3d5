// Sequencing reads for `call`: what the reference hands to `kmc -k<ref_k> -fm` (MALVA:104-110) -- FASTQ or (multi-line) FASTA,
// plain, gzip or BGZF (LineReader), one file, a comma-separated list (paired ends: counted together, as KMC counts them) or
// @list.txt (one path per line, KMC's convention).  The records' sequences are cut into chunks of WHOLE records with a '\n'
// between two of them, in pinned staging buffers, for mg_reads_add: the byte outside ACGT keeps every window inside its
// record.  A record longer than a chunk (a FASTA contig) continues in the next chunk behind its last ref_k - 1 bases, so each
// of its windows lies whole in exactly one chunk.
#pragma once
#include <sys/stat.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "io.hpp"

namespace malva {

inline bool reads_is_file(const std::string &p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// first non-blank byte of a file after decompression (0: none)
inline char reads_first_byte(const std::string &path)
{
    LineReader in(path);
    if (!in.ok()) return 0;
    std::string line;
    for (int i = 0; i < 64 && in.next(line); ++i)
        for (char ch : line)
            if (ch != ' ' && ch != '\t' && ch != '\r') return ch;
    return 0;
}

// Is `arg` reads (detection steps 3 and 4 of `call`; the KMC database and <prefix>.txt come first)?  *files = the paths.
inline bool reads_input(const std::string &arg, std::vector<std::string> *files)
{
    files->clear();
    if (arg.size() > 1 && arg[0] == '@' && !reads_is_file(arg) && reads_is_file(arg.substr(1))) {
        LineReader in(arg.substr(1));
        std::string line;
        while (in.next(line)) {
            const size_t a = line.find_first_not_of(" \t"), b = line.find_last_not_of(" \t");
            if (a != std::string::npos) files->push_back(line.substr(a, b - a + 1));
        }
        if (files->empty()) throw std::runtime_error("ERROR: " + arg.substr(1) + " lists no read files");
        return true;
    }
    if (arg.find(',') != std::string::npos && !reads_is_file(arg)) {
        size_t at = 0;
        for (;;) {
            const size_t c = arg.find(',', at);
            const std::string p = arg.substr(at, c == std::string::npos ? std::string::npos : c - at);
            if (!p.empty()) files->push_back(p);
            if (c == std::string::npos) break;
            at = c + 1;
        }
        return !files->empty();
    }
    if (!reads_is_file(arg)) return false;
    const char b = reads_first_byte(arg);
    if (b != '>' && b != '@') return false;
    files->push_back(arg);
    return true;
}

// One file's records: on_seq(piece, n) for the sequence bytes (a FASTA record in several pieces, one per line), on_end() after
// each record.  FASTQ: four lines per record (`@` header, sequence, `+` line, quality -- a quality line that starts with `@`
// is still a quality line); blank lines between records and `\r` line ends are tolerated; anything else malformed is an error
// that names the file and the line.  Stops after max_records records (0: all).
inline void reads_parse(const std::string &path, const std::function<void(const char *, size_t)> &on_seq, const std::function<void()> &on_end,
                        size_t max_records = 0)
{
    LineReader in(path);
    if (!in.ok()) throw std::runtime_error("ERROR: cannot open read file " + path);
    std::string line;
    size_t line_no = 0, records = 0;
    int fmt = 0; // '>' or '@' once the first record starts
    bool in_fasta_record = false;
    auto bad = [&](const std::string &what) { throw std::runtime_error("ERROR: " + path + ":" + std::to_string(line_no) + ": malformed FASTQ: " + what); };
    while (in.next(line)) {
        ++line_no;
        if (!fmt) {
            if (line.find_first_not_of(" \t") == std::string::npos) continue;
            if (line[0] != '>' && line[0] != '@') throw std::runtime_error("ERROR: " + path + ":" + std::to_string(line_no) + ": neither FASTA ('>') nor FASTQ ('@')");
            fmt = line[0];
        }
        if (fmt == '>') {
            if (line.empty()) continue;
            if (line[0] == '>') {
                if (in_fasta_record) {
                    on_end();
                    if (max_records && ++records >= max_records) return;
                }
                in_fasta_record = true;
                continue;
            }
            on_seq(line.data(), line.size());
            continue;
        }
        // FASTQ
        if (line.empty()) continue; // (between records)
        if (line[0] != '@') bad("expected a record header starting with '@'");
        if (!in.next(line)) {
            ++line_no;
            bad("the file ends after a record header");
        }
        ++line_no;
        const std::string seq = line;
        if (!in.next(line)) {
            ++line_no;
            bad("the file ends after a sequence line (no '+' line)");
        }
        ++line_no;
        if (line.empty() || line[0] != '+') bad("expected the '+' line after the sequence line");
        if (!in.next(line)) {
            ++line_no;
            bad("the file ends before the quality line");
        }
        ++line_no;
        if (line.size() != seq.size()) bad("quality line of " + std::to_string(line.size()) + " bytes for a sequence of " + std::to_string(seq.size()));
        on_seq(seq.data(), seq.size());
        on_end();
        if (max_records && ++records >= max_records) return;
    }
    if (in_fasta_record) on_end();
}

// The head of every FASTQ file checked before any device is created: a file that is not reads fails here, at once.
inline void reads_check_heads(const std::vector<std::string> &files)
{
    for (const auto &f : files) reads_parse(f, [](const char *, size_t) {}, [] {}, 4096);
}

// Chunks of whole records in pinned buffers (alloc / free: mg_host_alloc / mg_host_free), one reader thread per file, handed to
// `consume` on the calling thread in the order they fill.  At most `n_bufs` chunks exist at once.
struct ReadsChunker {
    size_t chunk_bytes = 32u << 20;
    unsigned ref_k = 43;
    std::function<void *(size_t)> alloc;
    std::function<void(void *)> release;

    void run(const std::vector<std::string> &files, const std::function<void(const char *, size_t)> &consume)
    {
        const size_t n_bufs = files.size() + 2;
        std::mutex mu;
        std::condition_variable cv;
        std::vector<char *> free_bufs, all_bufs;
        std::deque<std::pair<char *, size_t>> full;
        size_t done_files = 0;
        std::string error;
        for (size_t i = 0; i < n_bufs; ++i) {
            char *b = (char *)alloc(chunk_bytes);
            if (!b) {
                for (char *q : all_bufs) release(q);
                throw std::runtime_error("cannot allocate pinned staging for the reads");
            }
            all_bufs.push_back(b);
            free_bufs.push_back(b);
        }
        auto take_buf = [&]() -> char * {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return !free_bufs.empty() || !error.empty(); });
            if (!error.empty()) throw std::runtime_error(error);
            char *b = free_bufs.back();
            free_bufs.pop_back();
            return b;
        };
        auto worker = [&](const std::string &path) {
            try {
                char *buf = take_buf();
                size_t n = 0, rec_start = 0;
                auto emit = [&]() {
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        full.emplace_back(buf, n);
                    }
                    cv.notify_all();
                    buf = take_buf();
                    n = 0;
                    rec_start = 0;
                };
                auto on_seq = [&](const char *p, size_t len) {
                    while (len) {
                        size_t room = chunk_bytes - 1 - n; // (one byte kept for the record's separator)
                        if (room == 0) { // the record continues in the next chunk behind its last ref_k - 1 bases
                            const size_t ov = std::min<size_t>(ref_k - 1, n - rec_start);
                            std::string tail(buf + n - ov, ov);
                            emit();
                            memcpy(buf, tail.data(), ov);
                            n = ov;
                            continue;
                        }
                        const size_t take = std::min(room, len);
                        memcpy(buf + n, p, take);
                        n += take;
                        p += take;
                        len -= take;
                    }
                };
                auto on_end = [&]() {
                    buf[n++] = '\n';
                    rec_start = n;
                    if (chunk_bytes - n < 4096) emit();
                };
                reads_parse(path, on_seq, on_end);
                {
                    std::lock_guard<std::mutex> lk(mu);
                    if (n) full.emplace_back(buf, n);
                    else free_bufs.push_back(buf);
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                if (error.empty()) error = e.what();
            }
            std::lock_guard<std::mutex> lk(mu);
            ++done_files;
            cv.notify_all();
        };
        std::vector<std::thread> pool;
        for (const auto &f : files) pool.emplace_back(worker, f);
        std::string consume_error;
        for (;;) {
            std::pair<char *, size_t> c;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !full.empty() || done_files == files.size(); });
                if (full.empty()) break;
                c = full.front();
                full.pop_front();
            }
            try {
                if (consume_error.empty() && error.empty()) consume(c.first, c.second);
            } catch (const std::exception &e) {
                consume_error = e.what();
                std::lock_guard<std::mutex> lk(mu);
                if (error.empty()) error = e.what(); // (the readers stop at their next buffer)
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                free_bufs.push_back(c.first);
            }
            cv.notify_all();
        }
        for (auto &t : pool) t.join();
        for (char *q : all_bufs) release(q);
        if (!error.empty()) throw std::runtime_error(error);
    }
};

} // namespace malva
