// host_util.hpp -- small things the host side uses everywhere: integer knobs from the environment, the trace switch, a
// power of two, and the two thread helpers of the table builds.  PURE HOST C++17 (no HIP).
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace spm_hip
{

inline int env_int(const char *name, int dflt)
{
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}

// SPM_HIP_TRACE=1: one stderr line per C-ABI call that does work, and per index build, with its timings
inline bool trace_on()
{
    const char *v = getenv("SPM_HIP_TRACE");
    return v && *v && *v != '0';
}

inline uint32_t next_pow2(uint32_t x)
{
    uint32_t p = 1;
    while (p < x)
        p <<= 1;
    return p;
}

// A team of worker threads that lives as long as one index build: run(n, fn) calls fn(begin, end, thread) over [0, n) in
// contiguous slices, one per thread (the caller takes slice 0).  The rounds of dense_share_bits start 64 of these; spawning
// threads for each would cost more than the work.
class thread_team
{
  public:
    explicit thread_team(unsigned n) : n_(std::max(1u, n))
    {
        for (unsigned t = 1; t < n_; ++t)
            workers_.emplace_back([this, t]() { loop(t); });
    }
    ~thread_team()
    {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
            ++epoch_;
        }
        cv_.notify_all();
        for (std::thread &w : workers_)
            w.join();
    }
    unsigned size() const { return n_; }
    template <typename F>
    void run(size_t n, F fn)
    {
        if (n_ <= 1 || n < 2) {
            fn((size_t)0, n, 0u);
            return;
        }
        std::function<void(unsigned)> job = [&](unsigned t) { fn(n * t / n_, n * (t + 1) / n_, t); };
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = &job;
            pending_ = n_ - 1;
            ++epoch_;
        }
        cv_.notify_all();
        job(0);
        std::unique_lock<std::mutex> g(m_);
        done_.wait(g, [&]() { return pending_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(unsigned t)
    {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(unsigned)> *job = nullptr;
            {
                std::unique_lock<std::mutex> g(m_);
                cv_.wait(g, [&]() { return epoch_ != seen; });
                seen = epoch_;
                if (stop_)
                    return;
                job = job_;
            }
            (*job)(t);
            {
                std::lock_guard<std::mutex> g(m_);
                if (--pending_ == 0)
                    done_.notify_one();
            }
        }
    }
    unsigned n_;
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(unsigned)> *job_ = nullptr;
    unsigned pending_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

// fn(begin, end, thread) over [0, n) in contiguous slices, by a team of its own
template <typename F>
inline void parallel_slices(size_t n, unsigned n_threads, F fn)
{
    thread_team(n < 2 ? 1u : n_threads).run(n, fn);
}

} // namespace spm_hip
