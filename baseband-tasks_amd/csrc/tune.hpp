// How the plans that choose among candidate kernels (bbt_hip.hip: chan_pick, pfb_pick) time them,
// and how they remember the choice.  Host code with device calls; included by bbt_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace bbt {

// Scratch device memory of those plans: ONE buffer per device, allocated when the first such plan
// is made, grown when a plan needs more, and kept -- mapping and unmapping a GiB per plan preempts
// every queue of the process and took 0.3-2 s each after a few dozen plans.  1 GiB each way when
// the card has it to spare (well past the 256 MiB memory-side cache: at 256 MiB each way 1536
// channels ranked wrongly), at most an eighth of what is free; BBT_TUNE_KEEP=0 frees it after
// every plan (bbt_tune_scratch reports and frees it).
struct TuneScratch {
    std::mutex mu;
    std::map<int, std::pair<void*, size_t>> buf;         // device -> (pointer, bytes)
};
static inline TuneScratch& tune_scratch() {
    static TuneScratch* t = new TuneScratch;              // (never destroyed: the runtime may be gone by then)
    return *t;
}

// One comparison: holds the scratch buffer -- and with it the process-wide mutex, so such plans
// are made one at a time -- from construction to destruction.  The first `zeroed` bytes are the
// input of the candidates.  Everything runs on the null stream (a stream of its own would be one
// more hardware queue made and destroyed per plan), from HBM as in use.
class TuneBench {
  public:
    // A buffer of at least `least` bytes (as much as `want` if the card has it to spare), of which
    // `zeroed(size)` bytes are cleared; then the events, then the device is drained.
    template <class Zeroed>
    TuneBench(size_t least, size_t want, Zeroed zeroed) : lock_(tune_scratch().mu) {
        acquire(least, want);
        ready_ = base_ && hipMemsetAsync(base_, 0, zeroed(size_), nullptr) == hipSuccess &&
                 hipEventCreate(&e0_) == hipSuccess && hipEventCreate(&e1_) == hipSuccess &&
                 hipDeviceSynchronize() == hipSuccess;
    }
    TuneBench(const TuneBench&) = delete;
    TuneBench& operator=(const TuneBench&) = delete;
    ~TuneBench() {
        if (e0_) hipEventDestroy(e0_);
        if (e1_) hipEventDestroy(e1_);
        if (base_ && getenv("BBT_TUNE_KEEP") && !strcmp(getenv("BBT_TUNE_KEEP"), "0")) {
            auto& slot = tune_scratch().buf[dev_];
            if (slot.first) hipFree(slot.first);
            slot = {nullptr, 0};
        }
        if (!ready_) hipGetLastError();                   // (the failure is not the error of a later call)
    }
    bool ready() const { return ready_; }
    char* base() const { return base_; }
    size_t size() const { return size_; }
    // Milliseconds of run(stream) -- 0 = ok --, the better of two after a warm-up (code object
    // upload, tables); 1e30f if any step fails.
    template <class Run>
    float best_of(Run run) {
        float best = 1e30f;
        if (!ready_ || run((hipStream_t) nullptr)) return best;
        for (int r = 0; r < 2; ++r) {
            float ms = 0.f;
            if (hipEventRecord(e0_, nullptr) != hipSuccess || run((hipStream_t) nullptr) ||
                hipEventRecord(e1_, nullptr) != hipSuccess || hipEventSynchronize(e1_) != hipSuccess ||
                hipEventElapsedTime(&ms, e0_, e1_) != hipSuccess)
                return 1e30f;
            best = std::min(best, ms);
        }
        return best;
    }

  private:
    void acquire(size_t least, size_t want) {
        if (hipGetDevice(&dev_) != hipSuccess) return;
        auto& slot = tune_scratch().buf[dev_];
        if (slot.second < least) {
            if (slot.first) hipFree(slot.first);
            slot = {nullptr, 0};
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
            const size_t bytes = std::max(least, std::min(want, free_b / 4));
            void* ptr = nullptr;
            if (bytes > free_b / 2 || hipMalloc(&ptr, bytes) != hipSuccess) {
                hipGetLastError();
                return;
            }
            slot = {ptr, bytes};
        }
        base_ = (char*)slot.first;
        size_ = slot.second;
    }
    std::unique_lock<std::mutex> lock_;
    int dev_ = 0;
    char* base_ = nullptr;
    size_t size_ = 0;
    hipEvent_t e0_ = nullptr, e1_ = nullptr;
    bool ready_ = false;
};

// What a plan chose, remembered for the process: key -> choice.
template <class Key, class Choice>
class TuneMemo {
  public:
    bool find(const Key& key, Choice* choice) {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = map_.find(key);
        if (it == map_.end()) return false;
        *choice = it->second;
        return true;
    }
    void remember(const Key& key, const Choice& choice) {
        std::lock_guard<std::mutex> lock(mu_);
        map_[key] = choice;
    }

  private:
    std::mutex mu_;
    std::map<Key, Choice> map_;
};

}  // namespace bbt
