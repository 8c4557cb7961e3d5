// A context of libmalva_hip.so as the host driver holds it, and the host-side timers (MALVA_GENO_TIMERS)
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/malva_hip.h"

namespace malva {

// MALVA_GENO_TIMERS=1: where the host threads spend their time, summed per label, printed at exit (profiles/*cli*)
struct Timers {
    bool on = getenv("MALVA_GENO_TIMERS") != nullptr;
    std::mutex mu;
    std::map<std::string, double> acc;
    void add(const char *what, double s)
    {
        std::lock_guard<std::mutex> lk(mu);
        acc[what] += s;
    }
    ~Timers()
    {
        if (!on) return;
        for (const auto &kv : acc) fprintf(stderr, "[malva-geno/timer] %-28s %.3fs\n", kv.first.c_str(), kv.second);
    }
};
inline Timers g_timers;
struct Timed {
    const char *what;
    std::chrono::steady_clock::time_point t0;
    explicit Timed(const char *w) : what(w), t0(std::chrono::steady_clock::now()) {}
    ~Timed()
    {
        if (g_timers.on) g_timers.add(what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
};

struct Device {
    mg_ctx *ctx = nullptr;
    std::mutex mu; // calls on one context are serialised by the caller (include/malva_hip.h): held by whoever drives the context from a second thread
    ~Device() { mg_destroy(ctx); }
    void check(int rc, const char *what)
    {
        if (rc != MG_OK) throw std::runtime_error(std::string(what) + ": " + mg_last_error(ctx));
    }
};

// A call that fills `buf` and says in *need what it takes (mg_format_calls, mg_format_site_info, mg_encode_calls_bcf): made again with
// the buffer grown while it answers MG_ERR_LIMIT with a larger need -> its last return code
template <class Call> int call_grown(std::vector<char> &buf, Call call)
{
    for (;;) {
        uint64_t need = 0;
        const int rc = call(&need);
        if (rc != MG_ERR_LIMIT || need <= buf.size()) return rc;
        buf.resize(need);
    }
}

} // namespace malva
