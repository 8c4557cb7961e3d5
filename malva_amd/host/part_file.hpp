// part_file.hpp -- an output that exists under its name only when it is complete: PATH is written as PATH.part and takes its name in
// finish(); whatever is left of PATH.part goes with the object.  Two more kinds share the calls: a SCRATCH file keeps the name it was
// opened under, is closed by finish(), read again by a later pass and always removed with the object; STDOUT is flushed, never closed.
#pragma once
#include <cstdio>
#include <stdexcept>
#include <string>
#include <unistd.h>

struct PartFile {
    enum Kind { RENAMED, SCRATCH, STDOUT };
    std::string path, part; // part: what the destructor removes
    FILE *f = nullptr;
    Kind kind = RENAMED;
    PartFile() = default;
    PartFile(const PartFile &) = delete;
    PartFile &operator=(const PartFile &) = delete;
    void open(const std::string &p, Kind k = RENAMED)
    {
        path = p;
        kind = k;
        part = k == RENAMED ? p + ".part" : k == SCRATCH ? p : std::string();
        f = k == STDOUT ? stdout : fopen(part.c_str(), "wb");
        if (!f) {
            part.clear();
            throw std::runtime_error("cannot write " + path);
        }
    }
    // what: the message of a failure, where it is not "cannot write PATH"; a file that is not open takes nothing
    void write(const char *data, size_t n, const char *what = nullptr)
    {
        if (f && fwrite(data, 1, n, f) != n) throw std::runtime_error(what ? what : "cannot write " + path);
    }
    void write(const std::string &s, const char *what = nullptr) { write(s.data(), s.size(), what); }
    void close(const char *what = nullptr)
    {
        if (!f) return;
        FILE *closing = f;
        f = nullptr;
        if ((closing == stdout ? fflush(closing) : fclose(closing)) != 0) throw std::runtime_error(what ? what : "cannot write " + path);
    }
    // closed, then under its name (files of one set: close() them all first, then finish() them); a second call does nothing
    void finish(const char *what = nullptr)
    {
        close(what);
        if (kind != RENAMED || part.empty()) return;
        if (rename(part.c_str(), path.c_str()) != 0) throw std::runtime_error("cannot write " + path);
        part.clear();
    }
    ~PartFile()
    {
        if (f && f != stdout) fclose(f);
        if (!part.empty()) unlink(part.c_str());
    }
    static void put(const std::string &path, const std::string &text) // a whole file at once
    {
        PartFile file;
        file.open(path);
        file.write(text);
        file.finish();
    }
};
