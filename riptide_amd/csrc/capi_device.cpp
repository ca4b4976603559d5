// The globals of capi_device.hpp and the entry points that are about them:
// the thread's device, the library version, the launch profiler.
#include "capi_device.hpp"

namespace rt {

std::mutex g_mu;
Profiler g_prof;

int& current_device()
{
    thread_local int device = 0;
    return device;
}

Context& context()
{
    static std::vector<Context*> ctx;
    const int device = current_device();
    ck(hipSetDevice(device), "hipSetDevice");
    if ((int)ctx.size() <= device) ctx.resize(device + 1, nullptr);
    if (!ctx[device]) {
        Context* c = new Context();
        c->device = device;
        ck(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
        ctx[device] = c;
    }
    return *ctx[device];
}

ProfScope::ProfScope(hipStream_t s, int kind, bool enable) : s_(s), kind_(kind), open_(enable)
{
    if (!open_) return;
    {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        r_.a = g_prof.ev();
        try {
            r_.b = g_prof.ev();
        } catch (...) {
            g_prof.pool.push_back(r_.a);
            throw;
        }
    }
    if (hipError_t e = hipEventRecord(r_.a, s_)) {
        release();
        ck(e, "hipEventRecord");
    }
}

ProfScope::~ProfScope()
{
    if (open_) release();
}

void ProfScope::release()
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.pool.push_back(r_.a);
    g_prof.pool.push_back(r_.b);
    open_ = false;
}

void ProfScope::finish()
{
    if (!open_) return;
    ck(hipEventRecord(r_.b, s_), "hipEventRecord");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.rec[kind_].push_back(r_);
    open_ = false;
}

}  // namespace rt

using namespace rt;

extern "C" {

const char* rt_version(void) { return "riptide_amd 0.1.0 (gfx950)"; }

int rt_set_device(int device)
{
    return guarded([&] {
        ck(hipSetDevice(device), "hipSetDevice");
        current_device() = device;
        return RT_OK;
    });
}

int rt_profile_enable(int on)
{
    g_prof.on = on != 0;
    return RT_OK;
}

int rt_profile_reset(void)
{
    return guarded([&] {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        for (auto& v : g_prof.rec)
            for (auto& r : v) {
                g_prof.pool.push_back(r.a);
                g_prof.pool.push_back(r.b);
            }
        g_prof.rec[0].clear();
        g_prof.rec[1].clear();
        return RT_OK;
    });
}

int rt_profile_read(int kind, double* ms, double* alg, double* moved, uint64_t* launches)
{
    return guarded([&] {
        if (kind < 0 || kind > 1) throw std::invalid_argument("kind must be 0 or 1");
        std::lock_guard<std::mutex> lk(g_prof.mu);
        double t = 0, b = 0, mv = 0;
        for (auto& r : g_prof.rec[kind]) {
            ck(hipEventSynchronize(r.b), "hipEventSynchronize");
            float e = 0;
            ck(hipEventElapsedTime(&e, r.a, r.b), "hipEventElapsedTime");
            t += e;
            b += r.alg;
            mv += r.moved;
        }
        *ms = t;
        *alg = b;
        *moved = mv;
        *launches = g_prof.rec[kind].size();
        return RT_OK;
    });
}

}  // extern "C"
