// Device plumbing shared by the C ABI's device translation units
// (capi_*.cpp): the HIP error check, the per-device context of the host-buffer
// entry points, the thread's current device and the launch profiler.  Includes
// HIP; the one definition of each global is in capi_device.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_common.hpp"

namespace rt {

inline void ck(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e));
}

// ---- per-device context for host-buffer calls: stream + grow-only buffers
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    void* get(size_t n)
    {
        if (n > bytes) {
            if (p) (void)hipFree(p);
            p = nullptr;
            bytes = 0;
            ck(hipMalloc(&p, std::max<size_t>(n, 256)), "hipMalloc");
            bytes = std::max<size_t>(n, 256);
        }
        return p;
    }
};

struct Context {
    int device = -1;
    hipStream_t stream = nullptr;
    DevBuf buf[6];
};

extern std::mutex g_mu;    // guards every Context (one host-buffer call at a time)
int& current_device();     // the calling thread's device (rt_set_device)
Context& context();        // of the thread's device, made current; g_mu held

template <class T>
T* dev(Context& c, int slot, size_t count)
{
    return (T*)c.buf[slot].get(count * sizeof(T));
}

inline void h2d(void* d, const void* h, size_t bytes, hipStream_t s)
{
    if (bytes) ck(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
}

inline void d2h(void* h, const void* d, size_t bytes, hipStream_t s)
{
    if (bytes) ck(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
}

inline void sync(hipStream_t s) { ck(hipStreamSynchronize(s), "hipStreamSynchronize"); }

// Makes `device` current for a scope and restores the caller's device on
// exit: the side streams and events of a plan belong to the plan's device,
// whatever device the calling thread has current.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device)
    {
        int cur = 0;
        ck(hipGetDevice(&cur), "hipGetDevice");
        if (cur != device) {
            ck(hipSetDevice(device), "hipSetDevice");
            prev = cur;
        }
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- pinned staging of host tables for stream-ordered entry points
// A buffer belongs to the call that filled it until the stream has passed the
// copy out of it (its event); later calls reuse the buffers whose event has
// completed.  The buffers and their events live for the rest of the process.
struct PinnedStage {
    void* h = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    int device = 0;
    bool pending = false;
};

// a free buffer of `pool` of at least `bytes` on the current device, or a new
// one; the caller holds the pool's mutex, fills the buffer, queues the copy,
// sets `pending` and records `ev`
inline PinnedStage* pinned_stage_acquire(std::vector<PinnedStage*>& pool, size_t bytes)
{
    int device = 0;
    ck(hipGetDevice(&device), "hipGetDevice");
    for (PinnedStage* st : pool) {
        if (st->device != device || st->bytes < bytes) continue;
        if (st->pending && hipEventQuery(st->ev) != hipSuccess) continue;
        st->pending = false;
        return st;
    }
    std::unique_ptr<PinnedStage> st(new PinnedStage());
    st->device = device;
    st->bytes = std::max<size_t>(bytes, 4096);
    ck(hipHostMalloc(&st->h, st->bytes, hipHostMallocDefault), "hipHostMalloc");
    if (hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipHostFree(st->h);
        throw HipError("hipEventCreate failed");
    }
    pool.push_back(st.get());
    return st.release();
}

// ---- profiling of cone / downsample launches
struct ProfRec {
    hipEvent_t a, b;
    double alg, moved;
};
// One profiler per process, shared by every host thread (one per GPU is the
// supported model): `mu` guards the record lists and the event pool.
struct Profiler {
    std::mutex mu;
    std::atomic<bool> on{false};
    std::vector<ProfRec> rec[2];   // 0: cone launches, 1: ladders
    std::vector<hipEvent_t> pool;
    hipEvent_t ev()
    {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        ck(hipEventCreate(&e), "hipEventCreate");
        return e;
    }
};
extern Profiler g_prof;

// One profiling record around what a scope queues on a stream: two pooled
// events, the first recorded on construction, the second by finish(), which
// files the record under `kind`.  Left without finish() (an exception), the
// events go back to the pool and nothing is recorded.  Not enabled: no-op.
class ProfScope {
public:
    ProfScope(hipStream_t s, int kind, bool enable);
    ~ProfScope();
    bool on() const { return open_; }
    void add(double alg, double moved)
    {
        r_.alg += alg;
        r_.moved += moved;
    }
    void finish();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;

private:
    void release();
    hipStream_t s_;
    int kind_;
    bool open_;
    ProfRec r_{};
};

}  // namespace rt
