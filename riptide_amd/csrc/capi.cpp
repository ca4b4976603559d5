// C ABI of the engine (include/riptide_amd.h): host-buffer drop-ins for
// riptide.libcpp and the device-resident batched periodogram.
#include "riptide_amd.h"
#ifdef RT_TEST_HOOKS
#include "riptide_amd_test.h"
#endif

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_common.hpp"
#include "kernels.hpp"
#include "peaks_host.hpp"
#include "plan.hpp"

using namespace rt;

namespace {

thread_local int g_device = 0;

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

std::mutex g_mu;
std::vector<Context*> g_ctx;

Context& context()
{
    ck(hipSetDevice(g_device), "hipSetDevice");
    if ((int)g_ctx.size() <= g_device) g_ctx.resize(g_device + 1, nullptr);
    if (!g_ctx[g_device]) {
        Context* c = new Context();
        c->device = g_device;
        ck(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
        g_ctx[g_device] = c;
    }
    return *g_ctx[g_device];
}

template <class T>
T* dev(Context& c, int slot, size_t count)
{
    return (T*)c.buf[slot].get(count * sizeof(T));
}

void h2d(void* d, const void* h, size_t bytes, hipStream_t s)
{
    if (bytes) ck(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync H2D");
}

void d2h(void* h, const void* d, size_t bytes, hipStream_t s)
{
    if (bytes) ck(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
}

void sync(hipStream_t s) { ck(hipStreamSynchronize(s), "hipStreamSynchronize"); }

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

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
    std::vector<ProfRec> rec[2];
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
} g_prof;

#ifdef RT_TEST_HOOKS
// test builds only (libriptide_amd_testhooks.so): plans uploaded while set
// carry one corrupt unit (tests toggle it through rt_test_corrupt_next_plans)
std::atomic<int> g_test_corrupt{0};
#endif

// ---- a compiled plan resident on one device
// A side stream and events for co-scheduled pass sequences (run_cone_launches),
// taken by one call at a time from the plan's pool.
struct SideSet {
    hipStream_t s2 = nullptr;
    hipEvent_t err_join = nullptr;   // error path: joins s2 back into the caller's stream
    std::vector<hipEvent_t> ev;
};

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

struct DevicePlan {
    ExecPlan ex;
    UnitDesc* d_units = nullptr;
    uint32_t* d_blob = nullptr;     // tile-unit metadata (build_tile_blob)
    int device = 0;
    mutable std::mutex side_mu;
    mutable std::vector<std::unique_ptr<SideSet>> side_all;
    mutable std::vector<SideSet*> side_free;
    ~DevicePlan()
    {
        if (d_units) (void)hipFree(d_units);
        if (d_blob) (void)hipFree(d_blob);
        for (auto& ss : side_all) {
            for (hipEvent_t e : ss->ev) (void)hipEventDestroy(e);
            if (ss->err_join) (void)hipEventDestroy(ss->err_join);
            if (ss->s2) (void)hipStreamDestroy(ss->s2);
        }
    }
    // A side stream and `events` events on the plan's device (created there
    // whatever the calling thread's current device is).
    SideSet* take_side(size_t events) const
    {
        std::lock_guard<std::mutex> lk(side_mu);
        DeviceGuard dg(device);
        SideSet* ss;
        if (!side_free.empty()) {
            ss = side_free.back();
            side_free.pop_back();
        } else {
            side_all.push_back(std::make_unique<SideSet>());
            ss = side_all.back().get();
            ck(hipStreamCreateWithFlags(&ss->s2, hipStreamNonBlocking), "hipStreamCreate");
            ck(hipEventCreateWithFlags(&ss->err_join, hipEventDisableTiming), "hipEventCreate");
        }
        while (ss->ev.size() < events) {
            hipEvent_t e;
            ck(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
            ss->ev.push_back(e);
        }
        return ss;
    }
    void give_side(SideSet* ss) const
    {
        std::lock_guard<std::mutex> lk(side_mu);
        side_free.push_back(ss);
    }
    void upload()
    {
        ck(hipGetDevice(&device), "hipGetDevice");
        std::vector<UnitDesc> u(ex.items.size());
        for (size_t i = 0; i < u.size(); ++i) {
            const ConeItem& it = ex.items[i];
            const FfaXform& X = ex.xf[it.xform];
            UnitDesc d{};
            d.node_start = it.node_start;
            d.node_size = it.node_size;
            d.s0 = it.s0;
            d.s1 = it.s1;
            d.p = X.p;
            d.m = X.m;
            d.rows_eval = X.rows_eval;
            d.stdnoise = X.stdnoise;
            d.src_off = X.src_off;
            d.buf_off = X.buf_off;
            d.snr_row = X.snr_row;
            d.levels = it.levels;
            d.mode = it.mode;
            d.src = it.src;
            d.dst = it.dst;
            d.pad = it.pad;
            if (it.pad != kNoBlob) {
                const uint32_t* h = ex.blob.data() + it.pad;
                d.nruns = h[kHdrRuns];
                d.entries = h[kHdrEntries];
                d.nb = h[kHdrBottom];
                d.slot_words = h[kHdrSlotWords];
                d.run_off = h[kHdrRunOff];
                d.fill_chunks = h[kHdrFill];
                d.zero_row = h[kHdrZero];
            }
            u[i] = d;
        }
#ifdef RT_TEST_HOOKS
        // test-only hook (rt_test_corrupt_next_plans): give the first
        // whole-node unit more merge levels than any kernel instance runs,
        // after the host validation, so the kernel's own check refuses it and
        // sets the error flag (exercises rt_plan_check)
        if (g_test_corrupt.load(std::memory_order_relaxed) == 1)
            for (UnitDesc& d : u)
                if (d.mode == kModeWhole) {
                    d.levels = kMaxLevels + 1;
                    break;
                }
        // ... or (2) mark the first segmented-S/N final unit as a row-group
        // one: a unit of the other kind than its launch's kernel instance
        if (g_test_corrupt.load(std::memory_order_relaxed) == 2)
            for (UnitDesc& d : u)
                if (d.dst == kSelSnrSeg) {
                    d.dst = kSelSnr;
                    break;
                }
#endif
        ck(hipMalloc(&d_blob, std::max<size_t>(4, ex.blob.size()) * sizeof(uint32_t)), "hipMalloc");
        if (!ex.blob.empty())
            ck(hipMemcpy(d_blob, ex.blob.data(), ex.blob.size() * sizeof(uint32_t), hipMemcpyHostToDevice),
               "upload blob");
        ck(hipMalloc(&d_units, std::max<size_t>(1, u.size()) * sizeof(UnitDesc)), "hipMalloc");
        if (!u.empty())
            ck(hipMemcpy(d_units, u.data(), u.size() * sizeof(UnitDesc), hipMemcpyHostToDevice), "upload units");
    }
};

// Per-phase cycle counters of the cone kernel (RT_STAMPS diagnostic builds).
unsigned long long* g_stamps = nullptr;
uint64_t g_stamp_units = 0;      // unit records written since the last reset
std::vector<uint64_t> g_stamp_launch;   // first record of each launch since the last reset

// Run all cone launches of an exec plan.
// One cone launch of a plan on stream s (profiling: HIP events around it
// unless `prof_each` is off).
void cone_launch(const DevicePlan& P, const Launch& L, ConeArgs a, uint32_t batch, hipStream_t s, bool prof_each)
{
    a.items = P.d_units + L.first;
    a.num_items = L.count;
    const uint64_t units = (uint64_t)L.count * batch;   // one workgroup per (item, trial)
    if (L.count > 0x7FFFFFFFu || batch > 65535u) throw std::invalid_argument("too many cone work units in one launch");
    // diagnostic builds: this launch's unit records follow the previous ones
    a.stamps = nullptr;
    if (g_stamps) {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        if (g_stamp_units + units <= kTimelineCap) {
            a.stamps = g_stamps + g_stamp_units * kStampRecWords;
            g_stamp_launch.push_back(g_stamp_units);
            g_stamp_units += units;
        }
    }
    ProfRec r{};
    const bool prof = g_prof.on && prof_each;
    if (prof) {
        {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            r.a = g_prof.ev();
            r.b = g_prof.ev();
        }
        r.alg = L.alg_bytes * batch;
        r.moved = L.moved_bytes * batch;
        ck(hipEventRecord(r.a, s), "hipEventRecord");
    }
    ck(launch_cone(a, L.smax, L.rw, L.wide_snr != 0, L.snr, s), "cone_kernel");
    if (prof) {
        ck(hipEventRecord(r.b, s), "hipEventRecord");
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.rec[0].push_back(r);
    }
}

// A side set taken from a plan's pool for one launch sequence: returned to
// the pool on every exit.  While `forked`, launches may be queued on the side
// stream that the caller's stream has not joined; an exception then joins
// them back (so the caller cannot reuse or free the workspace while the side
// stream still writes it) before the set goes back to the pool.
struct SideLease {
    const DevicePlan& P;
    SideSet* ss;
    hipStream_t s;
    bool forked = false;
    SideLease(const DevicePlan& plan, size_t events, hipStream_t caller) : P(plan), ss(plan.take_side(events)), s(caller) {}
    ~SideLease()
    {
        if (forked) {
            DeviceGuard dg(P.device);
            if (hipEventRecord(ss->err_join, ss->s2) != hipSuccess || hipStreamWaitEvent(s, ss->err_join, 0) != hipSuccess)
                (void)hipStreamSynchronize(ss->s2);
        }
        P.give_side(ss);
    }
    SideLease(const SideLease&) = delete;
    SideLease& operator=(const SideLease&) = delete;
};

// RIPTIDE_AMD_SINGLE_STREAM=1: every cone launch of a plan on the caller's
// stream, in plan order, one profiling record per launch (per-launch A/B
// measurements and the parity test of the two-stream scheduling).
bool single_stream_forced()
{
    const char* e = std::getenv("RIPTIDE_AMD_SINGLE_STREAM");
    return e && e[0] == '1';
}

// Trials per cone workgroup (ConeArgs::trials_per_wg): one workgroup runs an
// item for up to this many trials of the batch, its record, blob and roll
// table loaded once.  RIPTIDE_AMD_TRIALS_PER_WG overrides the default.
uint32_t cone_trials_per_wg()
{
    if (const char* e = std::getenv("RIPTIDE_AMD_TRIALS_PER_WG")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 1 && v <= 65535) return (uint32_t)v;
    }
    return kConeTrialsPerWg;
}

// Run all cone launches of an exec plan.  A plan with two scratch banks
// (ExecPlan::banks) runs its transform groups co-scheduled on two streams:
// group g on stream g mod 2, its merge-only launches starting once group g - 1
// has finished its own merge-only launches -- so group g's merge-only passes
// (latency / LDS bound) share the CUs with group g - 1's final passes (VALU
// bound: the fused S/N).  Profiling then records one event pair around the
// whole sequence (launches overlap) with their summed algorithmic bytes.
void run_cone_launches(const DevicePlan& P, ConeArgs a, uint32_t batch, hipStream_t s)
{
    a.batch = batch;
    a.trials_per_wg = cone_trials_per_wg();
    a.flags = kConeDefaultFeatures;
    if (const char* e = std::getenv("RIPTIDE_AMD_CONE_FLAGS")) a.flags = (uint32_t)std::strtoul(e, nullptr, 0);
    // the 4/5-slot instances have no dense per-level path since round 5: the
    // fused two-level merge is their only merge, so the bit cannot be turned
    // off (an A/B value without it would leave their units unwritten)
    a.flags |= kConeFuse2;
    a.blob = P.d_blob;
    const std::vector<Launch>& Ls = P.ex.launches;
    DeviceGuard dg(P.device);
    const bool single = single_stream_forced();
    if (single || P.ex.banks < 2 || P.ex.groups < 2) {
        bool multi = false;
        for (const Launch& L : Ls) multi = multi || L.smax != Ls.front().smax;
        if (!multi || single) {
            for (const Launch& L : Ls) cone_launch(P, L, a, batch, s, true);
            return;
        }
        // slot-width buckets on two streams: within a transform group the
        // launches of different slot widths belong to disjoint transforms
        // (independent pass chains), so the group's main bucket (most cells)
        // runs on s and the others on a side stream, joined at the group's
        // end (the next group reuses the scratch buffers).  Each chain's
        // launch drains fill with the other's units: cone ms per trial cfg2
        // 7.092 -> 7.072, cfg3 1.795 -> 1.776, cfg1 0.274 -> 0.260
        // (profiles/r04r_ab_*_bucketstreams.log); the cone time is then one
        // profiling record from the fork to the join.
        const uint32_t G = std::max<uint32_t>(P.ex.groups, 1);
        SideLease lease(P, 2 * (size_t)G, s);
        SideSet* const ss = lease.ss;
        ProfRec r{};
        const bool prof = g_prof.on;
        if (prof) {
            {
                std::lock_guard<std::mutex> lk(g_prof.mu);
                r.a = g_prof.ev();
                r.b = g_prof.ev();
            }
            for (const Launch& L : Ls) {
                r.alg += L.alg_bytes * batch;
                r.moved += L.moved_bytes * batch;
            }
            ck(hipEventRecord(r.a, s), "hipEventRecord");
        }
        size_t li = 0;
        for (uint32_t g = 0; g < G && li < Ls.size(); ++g) {
            size_t l1 = li;
            std::map<uint32_t, uint64_t> cells;
            while (l1 < Ls.size() && Ls[l1].group == Ls[li].group) cells[Ls[l1].smax] += Ls[l1].cells, ++l1;
            uint32_t mainb = Ls[li].smax;
            for (const auto& kv : cells) if (kv.second > cells[mainb]) mainb = kv.first;
            ck(hipEventRecord(ss->ev[2 * g], s), "hipEventRecord");
            ck(hipStreamWaitEvent(ss->s2, ss->ev[2 * g], 0), "hipStreamWaitEvent");
            lease.forked = true;
            for (; li < l1; ++li) cone_launch(P, Ls[li], a, batch, Ls[li].smax == mainb ? s : ss->s2, false);
            ck(hipEventRecord(ss->ev[2 * g + 1], ss->s2), "hipEventRecord");
            ck(hipStreamWaitEvent(s, ss->ev[2 * g + 1], 0), "hipStreamWaitEvent");
            lease.forked = false;
        }
        if (li != Ls.size()) throw std::runtime_error("cone launches out of group order");
        if (prof) {
            ck(hipEventRecord(r.b, s), "hipEventRecord");
            std::lock_guard<std::mutex> lk(g_prof.mu);
            g_prof.rec[0].push_back(r);
        }
        return;
    }
    const uint32_t G = P.ex.groups;
    SideLease lease(P, 2 + (size_t)G, s);
    SideSet* const ss = lease.ss;
    ProfRec r{};
    const bool prof = g_prof.on;
    if (prof) {
        {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            r.a = g_prof.ev();
            r.b = g_prof.ev();
        }
        for (const Launch& L : Ls) {
            r.alg += L.alg_bytes * batch;
            r.moved += L.moved_bytes * batch;
        }
        ck(hipEventRecord(r.a, s), "hipEventRecord");
    }
    hipEvent_t fork = ss->ev[0], join = ss->ev[1];
    ck(hipEventRecord(fork, s), "hipEventRecord");
    ck(hipStreamWaitEvent(ss->s2, fork, 0), "hipStreamWaitEvent");
    lease.forked = true;
    size_t li = 0;
    for (uint32_t g = 0; g < G; ++g) {
        hipStream_t st = (g & 1u) ? ss->s2 : s;
        if (g >= 1) ck(hipStreamWaitEvent(st, ss->ev[2 + g - 1], 0), "hipStreamWaitEvent");
        while (li < Ls.size() && Ls[li].group == g && !Ls[li].snr) cone_launch(P, Ls[li++], a, batch, st, false);
        ck(hipEventRecord(ss->ev[2 + g], st), "hipEventRecord");
        while (li < Ls.size() && Ls[li].group == g) cone_launch(P, Ls[li++], a, batch, st, false);
    }
    if (li != Ls.size()) throw std::runtime_error("cone launches out of group order");
    ck(hipEventRecord(join, ss->s2), "hipEventRecord");
    ck(hipStreamWaitEvent(s, join, 0), "hipStreamWaitEvent");
    lease.forked = false;
    if (prof) {
        ck(hipEventRecord(r.b, s), "hipEventRecord");
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.rec[0].push_back(r);
    }
}

// Single-transform FFA (ffa2 / benchmark_ffa2): in (device) -> out (device).
// d_flag: device int the cone kernel sets if a unit breaks its budget (the
// caller checks it after synchronising).  A plan built here is freed only
// after the stream has drained; a cached plan lives in the caller.
void ffa_device(const float* d_in, size_t rows, size_t cols, float* d_out, float* d_tmp, int* d_flag, hipStream_t s,
                DevicePlan* cached = nullptr)
{
    if (!rows || !cols) return;
    if (lds_row_capacity((uint32_t)cols) >= 3 && (uint64_t)rows * cols * 4u < kMaxBlockBytes) {
        DevicePlan local;
        DevicePlan& P = cached ? *cached : local;
        if (!cached || P.ex.launches.empty()) {
            FfaXform X{};
            X.p = (uint32_t)cols;
            X.m = (uint32_t)rows;
            build_exec_plan({X}, false, 0, ~0ull, P.ex);
            P.upload();
        }
        ConeArgs a{};
        a.leaves = d_in;
        a.ping = d_out;
        a.pong = d_tmp;
        a.error_flag = d_flag;
        run_cone_launches(P, a, 1, s);
        if (!cached) sync(s);   // `local` (and its unit table) is freed on return
        return;
    }
    // rows too wide for LDS: per-depth global-memory passes
    int depth = 0;
    while ((1ull << depth) < rows) ++depth;
    std::vector<std::vector<uint2>> levels(depth + 1);
    levels[0].push_back(make_uint2(0, (uint32_t)rows));
    for (int d = 0; d < depth; ++d)
        for (const uint2& n : levels[d]) {
            if (n.y <= 1) { levels[d + 1].push_back(n); continue; }
            const uint32_t h = n.y >> 1;
            levels[d + 1].push_back(make_uint2(n.x, h));
            levels[d + 1].push_back(make_uint2(n.x + h, n.y - h));
        }
    uint2* d_nodes = nullptr;
    ck(hipMalloc(&d_nodes, std::max<size_t>(1, rows) * sizeof(uint2)), "hipMalloc");
    const float* src = d_in;
    for (int d = depth - 1; d >= 0; --d) {
        float* dst = ((d % 2) == 0) ? d_out : d_tmp;
        ck(hipMemcpyAsync(d_nodes, levels[d].data(), levels[d].size() * sizeof(uint2), hipMemcpyHostToDevice, s),
           "nodes");
        ck(launch_ffa_level(src, dst, d_nodes, (uint32_t)levels[d].size(), (uint32_t)rows, (uint32_t)cols, s),
           "ffa_level");
        ck(hipStreamSynchronize(s), "sync");
        src = dst;
    }
    if (depth == 0) ck(hipMemcpyAsync(d_out, d_in, rows * cols * 4, hipMemcpyDeviceToDevice, s), "copy");
    ck(hipStreamSynchronize(s), "sync");
    (void)hipFree(d_nodes);
}

}  // namespace

// ---------------------------------------------------------------------------
// periodogram plan
// ---------------------------------------------------------------------------
struct rt_plan {
    PgramPlan pg;
    DevicePlan dp;
    std::vector<uint32_t> widths;
    uint32_t* d_widths = nullptr;
    // the ladder (plan.hpp plan_ladder), the device copies of its rung lists
    // and the per-rung kernel's blocks over `rungs` / `rungs_w`
    LadderPlan ladder;
    DsRung* d_rungs = nullptr;
    DsRung* d_rungs_f = nullptr;
    DsRung* d_rungs_w = nullptr;
    uint32_t ds_blocks = 0, ds_blocks_w = 0;
    int* d_flag = nullptr;   // sticky device error flag of the cone kernel (rt_plan_check reads and clears it)
    ~rt_plan()
    {
        if (d_rungs) (void)hipFree(d_rungs);
        if (d_rungs_f) (void)hipFree(d_rungs_f);
        if (d_rungs_w) (void)hipFree(d_rungs_w);
        if (d_widths) (void)hipFree(d_widths);
        if (d_flag) (void)hipFree(d_flag);
    }
};

namespace {

rt_plan* make_plan(size_t size, double tsamp, const uint64_t* widths, size_t nw, double pmin, double pmax,
                   size_t bmin, size_t bmax)
{
    const PgramParams prm = checked_params(size, tsamp, pmin, pmax, bmin, bmax);
    const uint32_t wmax = checked_plan_widths(widths, nw, bmin);
    if (lds_row_capacity((uint32_t)bmax) < 3) throw std::invalid_argument("bins_max too large for the LDS FFA engine");
    // everything the host decides (plan.hpp); the rest of this function only uploads it
    HostPlan hp;
    plan_periodogram(prm, (uint32_t)nw, wmax, scratch_budget_floats(), cosched_banks(), hp);
    if (std::getenv("RIPTIDE_AMD_PER_RUNG_LADDER")) {   // every rung in the per-rung kernel (A/B runs, tests)
        hp.ladder.mode = kLadderPerRung;
        hp.ladder.margin = 0;
        hp.ladder.rungs_f.clear();
        hp.ladder.rungs_w.clear();
    }
    auto* P = new rt_plan();
    try {
        P->pg = std::move(hp.pg);
        P->dp.ex = std::move(hp.ex);
        P->ladder = std::move(hp.ladder);
        P->widths.assign(widths, widths + nw);
        ck(hipMalloc(&P->d_widths, std::max<size_t>(1, nw) * sizeof(uint32_t)), "hipMalloc");
        if (nw)
            ck(hipMemcpy(P->d_widths, P->widths.data(), nw * sizeof(uint32_t), hipMemcpyHostToDevice), "upload widths");
        P->dp.upload();
        ck(hipMalloc(&P->d_flag, sizeof(int)), "hipMalloc");
        ck(hipMemset(P->d_flag, 0, sizeof(int)), "hipMemset");
        const LadderPlan& l = P->ladder;
        for (const DsRung& d : l.rungs) P->ds_blocks += (uint32_t)((d.n + d.per_block - 1) / d.per_block);
        for (const DsRung& d : l.rungs_w) P->ds_blocks_w += (uint32_t)((d.n + d.per_block - 1) / d.per_block);
        auto upload = [](DsRung*& dst, const std::vector<DsRung>& src) {
            ck(hipMalloc(&dst, std::max<size_t>(1, src.size()) * sizeof(DsRung)), "hipMalloc");
            if (!src.empty())
                ck(hipMemcpy(dst, src.data(), src.size() * sizeof(DsRung), hipMemcpyHostToDevice), "upload rungs");
        };
        upload(P->d_rungs, l.rungs);
        if (l.mode != kLadderPerRung) upload(P->d_rungs_f, l.rungs_f);
        if (l.mode == kLadderHybrid) upload(P->d_rungs_w, l.rungs_w);
    } catch (...) {
        delete P;
        throw;
    }
    return P;
}

size_t plan_ws_bytes(const rt_plan* P, size_t batch)
{
    size_t b = align_up(P->pg.leaf_floats * 4 * batch, 256);
    b += 2 * align_up(P->dp.ex.scratch_floats * 4 * batch, 256);
    b += 256;   // slack
    return b;
}

// Workspace layout: [leaves | ping | pong]
struct PlanWs {
    float* leaves;
    float* ping;
    float* pong;
};

PlanWs plan_ws(const rt_plan* P, size_t batch, void* ws, size_t ws_bytes)
{
    if (ws_bytes < plan_ws_bytes(P, batch)) throw std::invalid_argument("workspace too small");
    char* w = (char*)ws;
    PlanWs o;
    o.leaves = (float*)w;
    w += align_up(P->pg.leaf_floats * 4 * batch, 256);
    o.ping = (float*)w;
    w += align_up(P->dp.ex.scratch_floats * 4 * batch, 256);
    o.pong = (float*)w;
    return o;
}

// The downsampling ladder of a batch into the workspace's leaf buffer.
void run_ladder(const rt_plan* P, const float* d_data, size_t batch, size_t data_stride, void* ws, size_t ws_bytes,
                hipStream_t s)
{
    float* const leaves = plan_ws(P, batch, ws, ws_bytes).leaves;
    ProfRec r{};
    const bool prof = g_prof.on;
    if (prof) {
        {
            std::lock_guard<std::mutex> lk(g_prof.mu);
            r.a = g_prof.ev();
            r.b = g_prof.ev();
        }
        ck(hipEventRecord(r.a, s), "hipEventRecord");
    }
    const LadderPlan& l = P->ladder;
    if (l.mode != kLadderPerRung)
        ck(launch_downsample_fused(d_data, P->pg.prm.size, data_stride, P->d_rungs_f, (uint32_t)l.rungs_f.size(),
                                   l.margin, leaves, P->pg.leaf_floats, (uint32_t)batch, s),
           "downsample_fused");
    if (l.mode == kLadderHybrid)
        ck(launch_downsample_ladder(d_data, P->pg.prm.size, data_stride, P->d_rungs_w, (uint32_t)l.rungs_w.size(),
                                    P->ds_blocks_w, leaves, P->pg.leaf_floats, (uint32_t)batch, s),
           "downsample_ladder");
    if (l.mode == kLadderPerRung)
        ck(launch_downsample_ladder(d_data, P->pg.prm.size, data_stride, P->d_rungs, (uint32_t)l.rungs.size(),
                                    P->ds_blocks, leaves, P->pg.leaf_floats, (uint32_t)batch, s),
           "downsample_ladder");
    if (prof) {
        ck(hipEventRecord(r.b, s), "hipEventRecord");
        // fused: the series is read once for its rungs; per-rung: once per rung
        double bytes = l.mode != kLadderPerRung ? 4.0 * P->pg.prm.size : 0.0;
        for (const DsRung& d : l.rungs) {
            const bool fused = rung_in_fused(l.mode, d);
            bytes += 4.0 * (double)d.n + (fused ? 0.0 : (d.identity ? 4.0 * d.n : 4.0 * P->pg.prm.size));
        }
        r.alg = r.moved = bytes * batch;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        g_prof.rec[1].push_back(r);
    }
}

// The FFA passes + fused S/N of a batch whose leaf buffer run_ladder filled.
void run_passes(const rt_plan* P, size_t batch, float* d_snrs, size_t snr_stride, void* ws, size_t ws_bytes,
                hipStream_t s)
{
    const PlanWs W = plan_ws(P, batch, ws, ws_bytes);
    float* const leaves = W.leaves;
    float* const ping = W.ping;
    float* const pong = W.pong;
    ConeArgs a{};
    a.num_widths = (uint32_t)P->widths.size();
    a.widths = P->d_widths;
    a.leaves = leaves;
    a.leaves_stride = P->pg.leaf_floats;
    a.ping = ping;
    a.pong = pong;
    a.buf_stride = P->dp.ex.scratch_floats;
    a.snr = d_snrs;
    a.snr_stride = snr_stride;
    a.error_flag = P->d_flag;
    run_cone_launches(P->dp, a, (uint32_t)batch, s);
}

void run_periodogram(const rt_plan* P, const float* d_data, size_t batch, size_t data_stride, float* d_snrs,
                     size_t snr_stride, void* ws, size_t ws_bytes, hipStream_t s)
{
    run_ladder(P, d_data, batch, data_stride, ws, ws_bytes, s);
    run_passes(P, batch, d_snrs, snr_stride, ws, ws_bytes, s);
}

// Dereddening + normalisation (device).  Workspace layout: [lores | rmed | partials]
struct DeredGeom {
    size_t sf = 1, n_lo = 0, rmed_w = 0;
    size_t lores_floats = 0, rmed_floats = 0, partial_doubles = 0;
    size_t slope_doubles = 0;   // np.interp segment slopes (sf > 1)
};
constexpr uint32_t kNormBlocks = 512;

DeredGeom dered_geom(size_t size, size_t ws, size_t minpts, size_t batch, bool deredden)
{
    DeredGeom g;
    if (deredden) {
        if (!(minpts % 2)) throw std::invalid_argument("min_points must be an odd number");
        const double q = (double)ws / (double)minpts;
        g.sf = (size_t)std::max(1.0, q);
        if (g.sf == 1) {
            g.n_lo = size;
            g.rmed_w = ws;
        } else {
            g.n_lo = size / g.sf;
            g.rmed_w = minpts;
            g.lores_floats = align_up(g.n_lo * batch, 64);
            g.slope_doubles = align_up(g.n_lo * batch, 32);
        }
        if (!(g.rmed_w % 2)) throw std::invalid_argument("width must be an odd number");
        if (!(g.rmed_w < g.n_lo)) throw std::invalid_argument("width must be < size");
        g.rmed_floats = align_up(g.n_lo * batch, 64);
    }
    // the unfused normalisation's partials, or the fused one's (two per
    // dereddening block: launch_deredden_normalise), then 2 * batch stats
    g.partial_doubles = std::max<size_t>((size_t)kNormBlocks, deredden ? 2 * dered_norm_blocks(size) : 0) * batch +
                        2 * batch + 8;
    return g;
}

size_t dered_ws_bytes(const DeredGeom& g)
{
    return (g.lores_floats + g.rmed_floats) * 4 + (g.slope_doubles + g.partial_doubles) * 8 + 256;
}

void run_deredden_normalise(const float* d_in, size_t size, size_t batch, size_t in_stride, const DeredGeom& g,
                            bool deredden, bool normalise, float* d_out, size_t out_stride, void* ws, hipStream_t s)
{
    float* lores = (float*)ws;
    float* rmed = lores + g.lores_floats;
    double* slopes = (double*)align_up((size_t)(rmed + g.rmed_floats), 256);
    double* partials = slopes + g.slope_doubles;
    const float* cur = d_in;
    size_t cur_stride = in_stride;
    const bool fused = deredden && normalise && g.sf > 1 &&
                       dered_norm_fusable(d_in, size, g.n_lo, (uint32_t)g.sf, d_out, in_stride, out_stride);
    if (deredden) {
        const float* rin = d_in;
        size_t rstride = in_stride;
        if (g.sf > 1) {
            ck(launch_scrunch(d_in, g.n_lo, (uint32_t)g.sf, lores, in_stride, g.n_lo, (uint32_t)batch, s), "scrunch");
            rin = lores;
            rstride = g.n_lo;
        }
        ck(launch_running_median(rin, g.n_lo, (uint32_t)g.rmed_w, rmed, rstride, g.n_lo, (uint32_t)batch, s),
           "running_median");
        if (fused) {
            const size_t np = 2 * dered_norm_blocks(size) * batch;
            ck(launch_deredden_normalise(d_in, size, rmed, g.n_lo, (uint32_t)g.sf, d_out, in_stride, g.n_lo,
                                         out_stride, (uint32_t)batch, s, slopes, partials, partials + np),
               "deredden_normalise");
            return;
        }
        ck(launch_deredden_subtract(d_in, size, rmed, g.n_lo, (uint32_t)g.sf, d_out, in_stride, g.n_lo, out_stride,
                                    (uint32_t)batch, s, g.slope_doubles ? slopes : nullptr),
           "deredden_subtract");
        cur = d_out;
        cur_stride = out_stride;
    }
    if (normalise) {
        ck(launch_normalise(cur, size, d_out, partials, kNormBlocks, cur_stride, out_stride, (uint32_t)batch, s),
           "normalise");
    } else if (!deredden && cur != d_out) {
        for (size_t b = 0; b < batch; ++b)
            ck(hipMemcpyAsync(d_out + b * out_stride, d_in + b * in_stride, size * 4, hipMemcpyDeviceToDevice, s),
               "copy");
    }
}

// ---- incoherent dedispersion: what the kernels' 32-bit indices and grids allow
void dedisp_check_shape(int dtype, size_t nsamp_blk, size_t nchans, size_t ndm, int64_t max_delay)
{
    if (dtype != RT_DEDISP_U8 && dtype != RT_DEDISP_I8 && dtype != RT_DEDISP_F32)
        throw std::invalid_argument("dedisperse: unknown sample type code");
    if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    if (dtype != RT_DEDISP_F32 && nchans > RT_DEDISP_MAX_CHANS_8BIT)
        throw std::invalid_argument("dedisperse: too many channels for an exact 8-bit sum (255 * nchans must be "
                                    "below 2^24)");
    if (nchans > 65535ull * 64) throw std::invalid_argument("dedisperse: too many channels");
    if (ndm > 65535ull * 16) throw std::invalid_argument("dedisperse: too many DMs for one call");
    if (nsamp_blk >= (1ull << 31)) throw std::invalid_argument("dedisperse: a block must be below 2^31 samples");
    if (max_delay < 0 || (uint64_t)max_delay >= nsamp_blk)
        throw std::invalid_argument("dedisperse: max_delay must be in [0, nsamp): the block is no longer than the "
                                    "largest delay");
}

// ---- candidate folding (folding.py:19-81)
// m and the mode / result rows of one candidate; throws as the header lists.
struct FoldShape {
    uint64_t m = 0;
    uint32_t mode = kFoldRows;
    uint64_t rows = 0;      // result rows (0: a 1-D profile)
    double vf = 0.0;
};

FoldShape fold_shape(size_t size, double f, size_t bins, size_t subints)
{
    if (!((f > 1.0) & (f <= (double)size)))
        throw std::invalid_argument("Downsampling factor must verify: 1 < f <= size");
    if (bins < 2) throw std::invalid_argument("fold: bins must be >= 2");
    if (bins > 0xFFFFFFFFull) throw std::invalid_argument("fold: too many bins");
    FoldShape s;
    s.m = downsampled_size(size, f) / bins;
    if (!s.m) throw std::invalid_argument("fold: no whole period fits in the data");
    if (s.m > 0xFFFFFFFFull) throw std::invalid_argument("fold: too many periods");
    if (subints > s.m) throw std::invalid_argument("fold: subints exceeds the number of whole periods");
    if (subints == 1 || s.m == 1) {
        s.mode = kFoldProfile;
    } else if (subints == 0 || subints == s.m) {
        s.rows = s.m;
    } else {
        s.mode = kFoldVertical;
        s.vf = (double)s.m / (double)subints;
        s.rows = downsampled_size(s.m, s.vf);
    }
    return s;
}

// The launch plan of one call: the rows table (every candidate), the subints
// table (those whose result is not the row array) and the workspace layout
// [both tables | row arrays of the subints candidates].
struct FoldPlan {
    std::vector<FoldCand> rows, sub;
    uint32_t rows_blocks = 0, sub_blocks = 0;
    size_t table_bytes = 0, ws_bytes = 0;
};

FoldPlan fold_plan(size_t size, const rt_fold_spec* specs, size_t nspecs)
{
    FoldPlan P;
    if (!nspecs) return P;
    if (!specs) throw std::invalid_argument("fold: null specs");
    uint64_t rb = 0, sb = 0, ws_floats = 0;
    P.rows.reserve(nspecs);
    for (size_t i = 0; i < nspecs; ++i) {
        const rt_fold_spec& sp = specs[i];
        const FoldShape sh = fold_shape(size, sp.factor, sp.bins, sp.subints);
        FoldCand c{};
        c.f = sp.factor;
        c.vf = sh.vf;
        c.n_rows_out = sh.m * (uint64_t)sp.bins;
        c.out_off = sp.out_off;
        c.scale = (float)std::pow((double)sh.m * sp.factor, -0.5);
        c.bins = sp.bins;
        c.m = (uint32_t)sh.m;
        c.mode = sh.mode;
        c.sub_rows = sh.mode == kFoldProfile ? 1u : (uint32_t)sh.rows;
        c.rows_in_ws = sh.mode != kFoldRows;
        c.rows_off = c.rows_in_ws ? ws_floats : sp.out_off;
        const uint32_t o = ds_per_block(sp.factor);
        c.staged = o >= 32;
        c.per_block = c.staged ? o : 256u;
        c.first_block = (uint32_t)rb;
        rb += (c.n_rows_out + c.per_block - 1) / c.per_block;
        if (rb > 0x7FFFFFFFull) throw std::invalid_argument("fold: too many outputs for one call");
        P.rows.push_back(c);
        if (c.rows_in_ws) {
            ws_floats += c.n_rows_out;
            FoldCand d = c;
            d.first_block = (uint32_t)sb;
            sb += ((uint64_t)c.sub_rows * c.bins + 255) / 256;
            P.sub.push_back(d);
        }
    }
    P.rows_blocks = (uint32_t)rb;
    P.sub_blocks = (uint32_t)sb;
    P.table_bytes = align_up((P.rows.size() + P.sub.size()) * sizeof(FoldCand), 256);
    P.ws_bytes = P.table_bytes + ws_floats * sizeof(float);
    return P;
}

size_t fold_result_floats(const FoldCand& c)
{
    return c.mode == kFoldRows ? c.n_rows_out : (size_t)c.sub_rows * c.bins;
}

// series indices, result ranges inside out_floats and disjoint
void fold_check_ranges(const FoldPlan& P, const rt_fold_spec* specs, size_t nseries, size_t out_floats)
{
    std::vector<std::pair<uint64_t, uint64_t>> rng;
    rng.reserve(P.rows.size());
    for (size_t i = 0; i < P.rows.size(); ++i) {
        if (specs[i].series >= nseries) throw std::invalid_argument("fold: series index out of range");
        const uint64_t lo = P.rows[i].out_off, len = fold_result_floats(P.rows[i]);
        if (lo > out_floats || len > out_floats - lo)
            throw std::invalid_argument("fold: result range exceeds the output buffer");
        rng.emplace_back(lo, lo + len);
    }
    std::sort(rng.begin(), rng.end());
    for (size_t i = 1; i < rng.size(); ++i)
        if (rng[i].first < rng[i - 1].second) throw std::invalid_argument("fold: result ranges overlap");
}

// Pinned staging buffers of the descriptor tables.  A buffer belongs to the
// call that filled it until the stream has passed the copy out of it (its
// event); later calls reuse the buffers whose event has completed.
struct FoldStage {
    void* h = nullptr;
    size_t bytes = 0;
    hipEvent_t ev = nullptr;
    int device = 0;
    bool pending = false;
};
std::mutex g_fold_mu;
std::vector<FoldStage*> g_fold_stages;

FoldStage* fold_stage_acquire(size_t bytes)   // g_fold_mu held
{
    int device = 0;
    ck(hipGetDevice(&device), "hipGetDevice");
    for (FoldStage* st : g_fold_stages) {
        if (st->device != device || st->bytes < bytes) continue;
        if (st->pending && hipEventQuery(st->ev) != hipSuccess) continue;
        st->pending = false;
        return st;
    }
    std::unique_ptr<FoldStage> st(new FoldStage());
    st->device = device;
    st->bytes = std::max<size_t>(bytes, 4096);
    ck(hipHostMalloc(&st->h, st->bytes, hipHostMallocDefault), "hipHostMalloc");
    if (hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipHostFree(st->h);
        throw HipError("hipEventCreate failed");
    }
    g_fold_stages.push_back(st.get());
    return st.release();
}

void run_fold(const FoldPlan& P, const rt_fold_spec* specs, const float* d_data, size_t size, size_t data_stride,
              float* d_out, void* d_ws, hipStream_t s)
{
    const size_t nr = P.rows.size(), ns = P.sub.size();
    FoldCand* d_rows = (FoldCand*)d_ws;
    FoldCand* d_sub = d_rows + nr;
    float* rows_ws = (float*)((char*)d_ws + P.table_bytes);
    {
        std::lock_guard<std::mutex> lk(g_fold_mu);
        FoldStage* st = fold_stage_acquire((nr + ns) * sizeof(FoldCand));
        FoldCand* h = (FoldCand*)st->h;
        for (size_t i = 0; i < nr; ++i) {
            h[i] = P.rows[i];
            h[i].src_off = (uint64_t)specs[i].series * data_stride;
        }
        for (size_t i = 0; i < ns; ++i) h[nr + i] = P.sub[i];
        ck(hipMemcpyAsync(d_rows, h, (nr + ns) * sizeof(FoldCand), hipMemcpyHostToDevice, s), "fold table H2D");
        st->pending = true;
        ck(hipEventRecord(st->ev, s), "hipEventRecord");
    }
    ck(launch_fold_rows(d_data, size, d_rows, (uint32_t)nr, P.rows_blocks, d_out, rows_ws, s), "fold_rows");
    ck(launch_fold_subints(d_sub, (uint32_t)ns, P.sub_blocks, d_out, rows_ws, s), "fold_subints");
}

// ---- harmonic flagging (harmonic.hpp, harmonic_kernels.hip)
static_assert(sizeof(HParams) == sizeof(rt_htest_params) && offsetof(HParams, denom_max) == offsetof(rt_htest_params, denom_max),
              "HParams is rt_htest_params");

// A tile of the pair matrix is at most kHTileWords 64-bit words (4 MiB)
// whatever n is: rows-per-tile = kHTileWords / ceil(n / 64), at least 1 since
// n <= kHMaxClusters.  Two tiles are in flight (one computing, one being
// resolved), each with a near list of kHNearCap pairs and a 16-byte header.
constexpr size_t kHTileWords = (size_t)1 << 19;
constexpr size_t kHMaxClusters = (size_t)1 << 24;
constexpr size_t kHDefaultRows = 1024;
constexpr uint32_t kHNearCap = 4096;
constexpr size_t kHHeaderBytes = 16;
constexpr size_t kHWordsOff = kHHeaderBytes + (size_t)kHNearCap * sizeof(uint2);
static_assert(kHMaxClusters / 64 <= kHTileWords, "one row fits a tile");

struct HStats {
    uint64_t tiles = 0, near_pairs = 0, host_rows = 0;
    double kernel_ms = 0;
};
thread_local HStats g_hstats;

struct HInputs {
    const double *freq, *snr, *ducy, *dm;
    HCand at(size_t i) const { return HCand{freq[i], snr[i], ducy[i], dm[i]}; }
};

HParams hparams_checked(const rt_htest_params* p)
{
    if (!p) throw std::invalid_argument("harmonics: null params");
    HParams P;
    std::memcpy(&P, p, sizeof P);
    if (!(P.tobs > 0.0)) throw std::invalid_argument("harmonics: tobs must be > 0");
    if (!hparams_ok(P)) throw std::invalid_argument("harmonics: denom_max must be in [1, 1024]");
    return P;
}

void hcheck_pairs(const HInputs& in, size_t n, const int32_t* pi, const int32_t* pj, size_t npairs)
{
    for (size_t k = 0; k < npairs; ++k) {
        if (pi[k] < 0 || pj[k] < 0 || (size_t)pi[k] >= n || (size_t)pj[k] >= n)
            throw std::invalid_argument("harmonics: pair index out of range");
        if (!hpair_ok(in.at(pi[k]), in.at(pj[k])))
            throw std::invalid_argument(
                "harmonics: freq and ducy must be finite and positive, the frequency ratio below 2^40");
    }
}

// pinned staging of the two tiles in flight and their events, per device;
// grow-only, kept for the rest of the process (guarded by g_mu)
struct HSlot {
    char* h = nullptr;
    hipEvent_t done = nullptr, k0 = nullptr, k1 = nullptr;
};
struct HStage {
    size_t bytes = 0;
    HSlot slot[2];
};
std::map<int, HStage> g_hstage;

HStage& harmonic_stage(int device, size_t bytes)
{
    HStage& st = g_hstage[device];
    for (HSlot& s : st.slot) {
        if (!s.done) {
            ck(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate");
            ck(hipEventCreate(&s.k0), "hipEventCreate");
            ck(hipEventCreate(&s.k1), "hipEventCreate");
        }
    }
    if (bytes > st.bytes) {
        for (HSlot& s : st.slot) {
            if (s.h) (void)hipHostFree(s.h);
            s.h = nullptr;
        }
        st.bytes = 0;
        for (HSlot& s : st.slot) ck(hipHostMalloc((void**)&s.h, bytes, hipHostMallocDefault), "hipHostMalloc");
        st.bytes = bytes;
    }
    return st;
}

void flag_harmonics(const HInputs& in, size_t n, const HParams& P, size_t block_rows, int32_t* parent, int64_t* hnum,
                    int64_t* hden)
{
    const size_t wpr = (n + 63) / 64;
    const size_t rows_cap = std::max<size_t>(1, kHTileWords / wpr);
    const size_t rows = std::min(block_rows ? block_rows : kHDefaultRows, rows_cap);
    const size_t nrows = n - 1;   // the last cluster has no pair to its right
    const size_t ntiles = (nrows + rows - 1) / rows;
    const size_t slot_bytes = kHWordsOff + std::min(rows, nrows) * wpr * sizeof(uint64_t);

    std::lock_guard<std::mutex> lk(g_mu);
    Context& c = context();
    double* din = dev<double>(c, 0, 4 * n);
    const double* src[4] = {in.freq, in.snr, in.ducy, in.dm};
    for (int a = 0; a < 4; ++a) h2d(din + a * n, src[a], n * sizeof(double), c.stream);
    char* dslot[2] = {(char*)c.buf[1].get(slot_bytes), (char*)c.buf[2].get(slot_bytes)};
    HStage& st = harmonic_stage(c.device, slot_bytes);

    auto issue = [&](size_t t) {
        HSlot& s = st.slot[t & 1];
        char* d = dslot[t & 1];
        const size_t i0 = t * rows, r = std::min(rows, nrows - i0);
        ck(hipMemsetAsync(d, 0, kHHeaderBytes, c.stream), "hipMemsetAsync");
        ck(hipEventRecord(s.k0, c.stream), "hipEventRecord");
        ck(launch_harmonic_pairs(din, din + n, din + 2 * n, din + 3 * n, (uint32_t)n, (uint32_t)i0, (uint32_t)r,
                                 (uint32_t)wpr, P, (uint64_t*)(d + kHWordsOff), (uint2*)(d + kHHeaderBytes), kHNearCap,
                                 (uint32_t*)d, c.stream),
           "harmonic_pairs");
        ck(hipEventRecord(s.k1, c.stream), "hipEventRecord");
        d2h(s.h, d, kHWordsOff + r * wpr * sizeof(uint64_t), c.stream);
        ck(hipEventRecord(s.done, c.stream), "hipEventRecord");
    };
    auto assign = [&](size_t i, size_t j) {
        const HDiag d = hdiag_pair(in.at(i), in.at(j), P);
        parent[j] = (int32_t)i;
        hnum[j] = d.num;
        hden[j] = d.den;
    };

    try {
        issue(0);
        for (size_t t = 0; t < ntiles; ++t) {
            if (t + 1 < ntiles) issue(t + 1);   // its slot held tile t - 1, resolved already
            HSlot& s = st.slot[t & 1];
            ck(hipEventSynchronize(s.done), "hipEventSynchronize");
            float ms = 0;
            ck(hipEventElapsedTime(&ms, s.k0, s.k1), "hipEventElapsedTime");
            g_hstats.kernel_ms += ms;
            g_hstats.tiles++;

            const size_t i0 = t * rows, r = std::min(rows, nrows - i0);
            const uint32_t count = *(const uint32_t*)s.h;
            const uint2* near = (const uint2*)(s.h + kHHeaderBytes);
            uint64_t* words = (uint64_t*)(s.h + kHWordsOff);
            const bool overflow = count > kHNearCap;
            if (!overflow) {
                // the host's verdict replaces the device's for every near pair
                for (uint32_t k = 0; k < count; ++k) {
                    const size_t i = near[k].x, j = near[k].y;
                    if (i < i0 || i >= i0 + r || j <= i || j >= n) throw std::runtime_error("harmonics: bad near pair");
                    uint64_t& w = words[(i - i0) * wpr + j / 64];
                    const uint64_t bit = (uint64_t)1 << (j % 64);
                    w = htest_pair(in.at(i), in.at(j), P, nullptr) ? (w | bit) : (w & ~bit);
                }
                g_hstats.near_pairs += count;
            }
            // rank order: a fundamental claims every unclaimed cluster related to it
            for (size_t i = i0; i < i0 + r; ++i) {
                if (parent[i] >= 0) continue;
                if (overflow) {
                    g_hstats.host_rows++;
                    for (size_t j = i + 1; j < n; ++j)
                        if (parent[j] < 0 && htest_pair(in.at(i), in.at(j), P, nullptr)) assign(i, j);
                    continue;
                }
                const uint64_t* row = words + (i - i0) * wpr;
                for (size_t w = i / 64; w < wpr; ++w) {
                    for (uint64_t bits = row[w]; bits; bits &= bits - 1) {
                        const size_t j = w * 64 + (size_t)__builtin_ctzll(bits);
                        if (j <= i || j >= n) throw std::runtime_error("harmonics: bit outside the upper triangle");
                        if (parent[j] < 0) assign(i, j);
                    }
                }
            }
        }
    } catch (...) {
        (void)hipStreamSynchronize(c.stream);   // nothing of this call stays in flight
        throw;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
extern "C" {

const char* rt_version(void) { return "riptide_amd 0.1.0 (gfx950)"; }

int rt_set_device(int device)
{
    return guarded([&] {
        ck(hipSetDevice(device), "hipSetDevice");
        g_device = device;
        return RT_OK;
    });
}

int rt_rollback(const float* x, size_t size, size_t shift, float* out)
{
    return guarded([&] {
        if (!size) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_rollback(dx, size, shift, nullptr, dz, c.stream), "rollback");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_fused_rollback_add(const float* x, const float* y, size_t size, size_t shift, float* out)
{
    return guarded([&] {
        if (!size) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dy = dev<float>(c, 1, size);
        float* dz = dev<float>(c, 2, size);
        h2d(dx, x, size * 4, c.stream);
        h2d(dy, y, size * 4, c.stream);
        ck(launch_rollback(dx, size, shift, dy, dz, c.stream), "fused_rollback_add");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_circular_prefix_sum(const float* x, size_t size, size_t nsum, float* out)
{
    return guarded([&] {
        if (!nsum) return RT_OK;
        if (!size) throw std::invalid_argument("circular_prefix_sum of an empty array");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, nsum + 1);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_circular_prefix_sum(dx, size, nsum, dz, c.stream), "circular_prefix_sum");
        d2h(out, dz, nsum * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_ffa2(const float* in, size_t rows, size_t cols, float* out)
{
    return guarded([&] {
        if (!rows || !cols) return RT_OK;
        if (rows > 0x7FFFFFFFull || rows * cols > (1ull << 40)) throw std::invalid_argument("ffa2 input too large");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        const size_t n = rows * cols;
        float* dx = dev<float>(c, 0, n);
        float* dz = dev<float>(c, 1, n);
        float* dt = dev<float>(c, 2, n);
        int* flag = dev<int>(c, 5, 1);
        ck(hipMemsetAsync(flag, 0, sizeof(int), c.stream), "hipMemsetAsync");
        h2d(dx, in, n * 4, c.stream);
        ffa_device(dx, rows, cols, dz, dt, flag, c.stream);
        int hflag = 0;
        d2h(&hflag, flag, sizeof hflag, c.stream);
        d2h(out, dz, n * 4, c.stream);
        sync(c.stream);
        if (hflag) throw std::runtime_error("cone kernel: work item exceeded the LDS budget");
        return RT_OK;
    });
}

int rt_benchmark_ffa2(size_t rows, size_t cols, size_t loops, double* seconds)
{
    return guarded([&] {
        *seconds = 0;
        if (!rows || !cols || !loops) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        const size_t n = rows * cols;
        float* dx = dev<float>(c, 0, n);
        float* dz = dev<float>(c, 1, n);
        float* dt = dev<float>(c, 2, n);
        int* flag = dev<int>(c, 5, 1);
        ck(hipMemsetAsync(dx, 0, n * 4, c.stream), "memset");
        ck(hipMemsetAsync(flag, 0, sizeof(int), c.stream), "hipMemsetAsync");
        DevicePlan P;
        ffa_device(dx, rows, cols, dz, dt, flag, c.stream, &P);   // warm-up + plan
        hipEvent_t a, b;
        ck(hipEventCreate(&a), "event");
        ck(hipEventCreate(&b), "event");
        ck(hipEventRecord(a, c.stream), "record");
        for (size_t i = 0; i < loops; ++i) ffa_device(dx, rows, cols, dz, dt, flag, c.stream, &P);
        ck(hipEventRecord(b, c.stream), "record");
        ck(hipEventSynchronize(b), "sync");
        float ms = 0;
        ck(hipEventElapsedTime(&ms, a, b), "elapsed");
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        int hflag = 0;
        ck(hipMemcpy(&hflag, flag, sizeof hflag, hipMemcpyDeviceToHost), "flag");
        if (hflag) throw std::runtime_error("cone kernel: work item exceeded the LDS budget");
        *seconds = ms * 1e-3 / (double)loops;
        return RT_OK;
    });
}

int rt_snr2(const float* x, size_t rows, size_t cols, const uint64_t* widths, size_t nw, float stdnoise, float* out)
{
    return guarded([&] {
        if (!(stdnoise > 0)) throw std::invalid_argument("stdnoise must be > 0");
        check_widths(widths, nw, cols);
        if (!rows || !nw) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        const size_t n = rows * cols;
        float* dx = dev<float>(c, 0, n);
        float* dc = dev<float>(c, 1, n + rows);
        uint32_t* dw = dev<uint32_t>(c, 2, nw);
        float* dz = dev<float>(c, 3, rows * nw);
        std::vector<uint32_t> w32(widths, widths + nw);
        h2d(dx, x, n * 4, c.stream);
        h2d(dw, w32.data(), nw * 4, c.stream);
        ck(launch_snr_rows(dx, rows, (uint32_t)cols, dw, (uint32_t)nw, stdnoise, dc, dz, c.stream), "snr");
        d2h(out, dz, rows * nw * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_snr1(const float* x, size_t size, const uint64_t* widths, size_t nw, float stdnoise, float* out)
{
    return rt_snr2(x, 1, size, widths, nw, stdnoise, out);
}

size_t rt_downsampled_size(size_t size, double f) { return downsampled_size(size, f); }

int rt_downsample(const float* x, size_t size, double f, float* out)
{
    return guarded([&] {
        // downsample.hpp:11-16
        if (!((f > 1.0) & (f <= (double)size)))
            throw std::invalid_argument("Downsampling factor must verify: 1 < f <= size");
        const size_t n = downsampled_size(size, f);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, n);
        DsRung* dr = dev<DsRung>(c, 2, 1);
        DsRung r{};
        r.f = f;
        r.n = n;
        r.first_block = 0;
        ds_configure(r);
        h2d(dx, x, size * 4, c.stream);
        h2d(dr, &r, sizeof r, c.stream);
        ck(launch_downsample_ladder(dx, size, size, dr, 1, (uint32_t)((n + r.per_block - 1) / r.per_block), dz, n,
                                    1, c.stream),
           "downsample");
        d2h(out, dz, n * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_downsample_rows(const float* x, size_t rows, size_t size, double f, float* out)
{
    return guarded([&] {
        if (!((f > 1.0) & (f <= (double)size)))
            throw std::invalid_argument("Downsampling factor must verify: 1 < f <= size");
        if (!rows) return RT_OK;
        if (rows > 65535) throw std::invalid_argument("at most 65535 rows per call");
        const size_t n = downsampled_size(size, f);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, rows * size);
        float* dz = dev<float>(c, 1, rows * n);
        DsRung* dr = dev<DsRung>(c, 2, 1);
        DsRung r{};
        r.f = f;
        r.n = n;
        r.first_block = 0;
        ds_configure(r);
        h2d(dx, x, rows * size * 4, c.stream);
        h2d(dr, &r, sizeof r, c.stream);
        ck(launch_downsample_ladder(dx, size, size, dr, 1, (uint32_t)((n + r.per_block - 1) / r.per_block), dz, n,
                                    (uint32_t)rows, c.stream),
           "downsample");
        d2h(out, dz, rows * n * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_fold_shape(size_t size, double factor, size_t bins, size_t subints, size_t* m, size_t* rows)
{
    return guarded([&] {
        const FoldShape s = fold_shape(size, factor, bins, subints);
        if (m) *m = s.m;
        if (rows) *rows = s.rows;
        return RT_OK;
    });
}

int rt_fold_workspace_bytes(size_t size, const rt_fold_spec* specs, size_t nspecs, size_t* bytes)
{
    return guarded([&] {
        const size_t need = fold_plan(size, specs, nspecs).ws_bytes;
        if (bytes) *bytes = need;
        return RT_OK;
    });
}

int rt_fold_device(const float* d_data, size_t size, size_t data_stride, size_t nseries, const rt_fold_spec* specs,
                   size_t nspecs, float* d_out, size_t out_floats, void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        if (!nspecs) return RT_OK;
        const FoldPlan P = fold_plan(size, specs, nspecs);
        fold_check_ranges(P, specs, nseries, out_floats);
        if (data_stride < size) throw std::invalid_argument("fold: data_stride is shorter than the series");
        if (ws_bytes < P.ws_bytes) throw std::invalid_argument("workspace too small");
        if (!d_data || !d_out || !d_ws) throw std::invalid_argument("fold: null device pointer");
        run_fold(P, specs, d_data, size, data_stride, d_out, d_ws, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_fold(const float* x, size_t size, size_t nseries, const rt_fold_spec* specs, size_t nspecs, float* out,
            size_t out_floats)
{
    return guarded([&] {
        if (!nspecs) return RT_OK;
        const FoldPlan P = fold_plan(size, specs, nspecs);
        fold_check_ranges(P, specs, nseries, out_floats);
        if (!x || !out) throw std::invalid_argument("fold: null buffer");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, nseries * size);
        float* dz = dev<float>(c, 1, out_floats);
        void* dw = c.buf[2].get(P.ws_bytes);
        h2d(dx, x, nseries * size * 4, c.stream);
        run_fold(P, specs, dx, size, size, dz, dw, c.stream);
        d2h(out, dz, out_floats * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

static void dedisp_check_flags(uint32_t flags)
{
    if (flags & ~RT_DEDISP_ZERO_DM) throw std::invalid_argument("dedisperse: unknown flag bit");
}

int rt_dedisperse_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, size_t* bytes)
{
    return rt_dedisperse_workspace_bytes_opt(dtype, nsamp_blk, nchans, 0u, bytes);
}

int rt_dedisperse_workspace_bytes_opt(int dtype, size_t nsamp_blk, size_t nchans, uint32_t flags, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("dedisperse: bytes is NULL");
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
        *bytes = (size_t)dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags);
        return RT_OK;
    });
}

int rt_dedisperse_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const int32_t* d_delays,
                         const uint8_t* d_mask, size_t ndm, int64_t max_delay, float* d_out, size_t out_stride,
                         size_t out_offset, void* d_ws, size_t ws_bytes, void* stream)
{
    return rt_dedisperse_device_opt(d_block, dtype, nsamp_blk, nchans, d_delays, d_mask, ndm, max_delay, d_out,
                                    out_stride, out_offset, d_ws, ws_bytes, stream, 0u);
}

int rt_dedisperse_device_opt(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                             const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, int64_t max_delay,
                             float* d_out, size_t out_stride, size_t out_offset, void* d_ws, size_t ws_bytes,
                             void* stream, uint32_t flags)
{
    return guarded([&] {
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp_blk, nchans, ndm, max_delay);
        const size_t nout = nsamp_blk - (size_t)max_delay;
        if (out_offset > out_stride || nout > out_stride - out_offset)
            throw std::invalid_argument("dedisperse: out_stride is shorter than out_offset plus the block's outputs");
        if (!d_block || !d_delays || !d_out || !d_ws) throw std::invalid_argument("dedisperse: null device pointer");
        if ((uintptr_t)d_ws % 16 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("dedisperse: misaligned device pointer");
        if (ws_bytes < dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags))
            throw std::invalid_argument("workspace too small");
        ck(launch_dedisperse(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_delays, d_mask, (uint32_t)ndm,
                             (uint32_t)max_delay, d_out + out_offset, out_stride, d_ws, flags, (hipStream_t)stream),
           "dedisperse");
        return RT_OK;
    });
}

int rt_dedisperse(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays, const uint8_t* mask,
                  size_t ndm, int64_t max_delay, float* out)
{
    return rt_dedisperse_opt(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, out, 0u);
}

int rt_dedisperse_opt(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                      const uint8_t* mask, size_t ndm, int64_t max_delay, float* out, uint32_t flags)
{
    return guarded([&] {
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp, nchans, ndm, max_delay);
        if (!x || !delays || !out) throw std::invalid_argument("dedisperse: null buffer");
        std::vector<int32_t> del(ndm * nchans);
        for (size_t i = 0; i < del.size(); ++i) {
            if (delays[i] < 0 || delays[i] > max_delay)
                throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
            del[i] = (int32_t)delays[i];
        }
        const size_t nout = nsamp - (size_t)max_delay;
        const size_t in_bytes = nsamp * nchans * (dtype == RT_DEDISP_F32 ? 4 : 1);
        const size_t ws_bytes = (size_t)dedisp_workspace_bytes(dtype, nsamp, nchans, flags);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        void* dx = c.buf[0].get(in_bytes);
        float* dz = dev<float>(c, 1, ndm * nout);
        void* dw = c.buf[2].get(ws_bytes);
        int32_t* dd = dev<int32_t>(c, 3, del.size());
        uint8_t* dm = mask ? dev<uint8_t>(c, 4, nchans) : nullptr;
        h2d(dx, x, in_bytes, c.stream);
        h2d(dd, del.data(), del.size() * 4, c.stream);
        if (mask) h2d(dm, mask, nchans, c.stream);
        ck(launch_dedisperse(dx, dtype, (uint32_t)nsamp, (uint32_t)nchans, dd, dm, (uint32_t)ndm,
                             (uint32_t)max_delay, dz, nout, dw, flags, c.stream),
           "dedisperse");
        d2h(out, dz, ndm * nout * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_zero_dm_mean_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const uint8_t* d_mask,
                           float* d_m, void* stream)
{
    return guarded([&] {
        dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
        if (!d_block || !d_m) throw std::invalid_argument("zero_dm_mean: null device pointer");
        if ((uintptr_t)d_m % 4 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("zero_dm_mean: misaligned device pointer");
        ck(launch_zero_dm_mean(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_mask, d_m,
                               (hipStream_t)stream),
           "zero_dm_mean");
        return RT_OK;
    });
}

// the statistics have no exactness limit on the channel count of 8-bit data
static void chanstats_check_shape(int dtype, size_t nsamp_blk, size_t nchans)
{
    dedisp_check_shape(RT_DEDISP_F32, nsamp_blk, nchans, 1, 0);
    if (dtype != RT_DEDISP_U8 && dtype != RT_DEDISP_I8 && dtype != RT_DEDISP_F32)
        throw std::invalid_argument("channel_stats: unknown sample type code");
}

int rt_channel_stats_workspace_bytes(size_t nsamp_blk, size_t nchans, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("channel_stats: bytes is NULL");
        chanstats_check_shape(RT_DEDISP_F32, nsamp_blk, nchans);
        *bytes = (size_t)chanstats_workspace_bytes(nsamp_blk, nchans);
        return RT_OK;
    });
}

int rt_channel_stats_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, double* d_acc,
                            void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        chanstats_check_shape(dtype, nsamp_blk, nchans);
        if (!d_block || !d_acc || !d_ws) throw std::invalid_argument("channel_stats: null device pointer");
        if ((uintptr_t)d_acc % 8 || (uintptr_t)d_ws % 8 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("channel_stats: misaligned device pointer");
        if (ws_bytes < chanstats_workspace_bytes(nsamp_blk, nchans))
            throw std::invalid_argument("workspace too small");
        ck(launch_channel_stats(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_acc, d_ws,
                                (hipStream_t)stream),
           "channel_stats");
        return RT_OK;
    });
}

int rt_hdiag_host(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                  const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params, int64_t* num,
                  int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance)
{
    return guarded([&] {
        const HParams P = hparams_checked(params);
        if (!npairs) return RT_OK;
        if (!freq || !snr || !ducy || !dm || !pi || !pj || !num || !den || !phase_distance || !dm_distance ||
            !snr_distance)
            throw std::invalid_argument("harmonics: null buffer");
        const HInputs in{freq, snr, ducy, dm};
        hcheck_pairs(in, n, pi, pj, npairs);
        for (size_t k = 0; k < npairs; ++k) {
            const HDiag d = hdiag_pair(in.at(pi[k]), in.at(pj[k]), P);
            num[k] = d.num;
            den[k] = d.den;
            phase_distance[k] = d.phase_distance;
            dm_distance[k] = d.dm_distance;
            snr_distance[k] = d.snr_distance;
        }
        return RT_OK;
    });
}

int rt_hdiag_pairs(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                   const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params, int64_t* num,
                   int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance)
{
    return guarded([&] {
        const HParams P = hparams_checked(params);
        if (!npairs) return RT_OK;
        if (!freq || !snr || !ducy || !dm || !pi || !pj || !num || !den || !phase_distance || !dm_distance ||
            !snr_distance)
            throw std::invalid_argument("harmonics: null buffer");
        const HInputs in{freq, snr, ducy, dm};
        hcheck_pairs(in, n, pi, pj, npairs);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        double* din = dev<double>(c, 0, 4 * n);
        int32_t* dp = dev<int32_t>(c, 1, 2 * npairs);
        int64_t* dout = dev<int64_t>(c, 2, 5 * npairs);   // num, den, then the three distances (8 bytes each)
        double* dd = (double*)(dout + 2 * npairs);
        const double* src[4] = {freq, snr, ducy, dm};
        for (int a = 0; a < 4; ++a) h2d(din + a * n, src[a], n * sizeof(double), c.stream);
        h2d(dp, pi, npairs * sizeof(int32_t), c.stream);
        h2d(dp + npairs, pj, npairs * sizeof(int32_t), c.stream);
        ck(launch_harmonic_diag(din, din + n, din + 2 * n, din + 3 * n, dp, dp + npairs, npairs, P, dout, dout + npairs,
                                dd, dd + npairs, dd + 2 * npairs, c.stream),
           "harmonic_diag");
        d2h(num, dout, npairs * 8, c.stream);
        d2h(den, dout + npairs, npairs * 8, c.stream);
        d2h(phase_distance, dd, npairs * 8, c.stream);
        d2h(dm_distance, dd + npairs, npairs * 8, c.stream);
        d2h(snr_distance, dd + 2 * npairs, npairs * 8, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_flag_harmonics(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                      const rt_htest_params* params, size_t block_rows, int32_t* parent, int64_t* hnum, int64_t* hden)
{
    return guarded([&] {
        g_hstats = HStats();
        if (n && (!parent || !hnum || !hden)) throw std::invalid_argument("harmonics: null buffer");
        for (size_t i = 0; i < n; ++i) {
            parent[i] = -1;
            hnum[i] = hden[i] = 0;
        }
        if (n <= 1) return RT_OK;
        if (!freq || !snr || !ducy || !dm) throw std::invalid_argument("harmonics: null buffer");
        const HParams P = hparams_checked(params);
        if (n > kHMaxClusters) throw std::invalid_argument("harmonics: more than 2^24 clusters");
        const HInputs in{freq, snr, ducy, dm};
        double lo = freq[0], hi = freq[0];
        for (size_t i = 0; i < n; ++i) {
            if (!hcand_ok(in.at(i))) throw std::invalid_argument("harmonics: freq and ducy must be finite and positive");
            lo = std::min(lo, freq[i]);
            hi = std::max(hi, freq[i]);
        }
        // IEEE division is monotonic: every pair's ratio is at most hi / lo
        if (!(hi / lo < kHRatioMax)) throw std::invalid_argument("harmonics: frequency ratios must be below 2^40");
        flag_harmonics(in, n, P, block_rows, parent, hnum, hden);
        return RT_OK;
    });
}

int rt_flag_harmonics_stats(uint64_t* tiles, uint64_t* near_pairs, uint64_t* host_rows, double* kernel_ms)
{
    if (tiles) *tiles = g_hstats.tiles;
    if (near_pairs) *near_pairs = g_hstats.near_pairs;
    if (host_rows) *host_rows = g_hstats.host_rows;
    if (kernel_ms) *kernel_ms = g_hstats.kernel_ms;
    return RT_OK;
}

int rt_periodogram(const float* data, size_t size, double tsamp, const uint64_t* widths, size_t nw, double pmin,
                   double pmax, size_t bmin, size_t bmax, double* periods, uint32_t* foldbins, float* snrs)
{
    return guarded([&] {
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        rt_plan* P = make_plan(size, tsamp, widths, nw, pmin, pmax, bmin, bmax);
        std::unique_ptr<rt_plan> hold(P);
        fill_grid(P->pg, periods, foldbins);
        const size_t L = P->pg.length;
        if (!L) return RT_OK;
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, std::max<size_t>(1, L * nw));
        void* ws = c.buf[2].get(plan_ws_bytes(P, 1));
        h2d(dx, data, size * 4, c.stream);
        run_periodogram(P, dx, 1, size, dz, L * nw, ws, plan_ws_bytes(P, 1), c.stream);
        int flag = 0;
        d2h(&flag, P->d_flag, sizeof flag, c.stream);
        d2h(snrs, dz, L * nw * 4, c.stream);
        sync(c.stream);
        if (flag) throw std::runtime_error("cone kernel: work item exceeded the LDS budget");
        return RT_OK;
    });
}

int rt_running_median(const float* x, size_t size, size_t width, float* out)
{
    return guarded([&] {
        // running_median.hpp:103-107
        if (!(width % 2)) throw std::invalid_argument("width must be an odd number");
        if (!(width < size)) throw std::invalid_argument("width must be < size");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_running_median(dx, size, (uint32_t)width, dz, size, size, 1, c.stream), "running_median");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_fast_running_median(const float* x, size_t size, size_t ws, size_t minpts, double* out)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, 1, true);
        if (g.sf == 1) throw std::invalid_argument("scrunch factor is 1: use rt_running_median");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        double* dz = dev<double>(c, 1, size);
        float* lores = dev<float>(c, 2, g.n_lo);
        float* rmed = dev<float>(c, 3, g.n_lo);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_scrunch(dx, g.n_lo, (uint32_t)g.sf, lores, size, g.n_lo, 1, c.stream), "scrunch");
        ck(launch_running_median(lores, g.n_lo, (uint32_t)g.rmed_w, rmed, g.n_lo, g.n_lo, 1, c.stream),
           "running_median");
        ck(launch_interp(size, rmed, g.n_lo, (uint32_t)g.sf, dz, c.stream), "interp");
        d2h(out, dz, size * 8, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_deredden_normalise(const float* x, size_t size, size_t ws, size_t minpts, int deredden, int normalise,
                          float* out)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, 1, deredden != 0);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        void* w = c.buf[2].get(dered_ws_bytes(g));
        h2d(dx, x, size * 4, c.stream);
        run_deredden_normalise(dx, size, 1, size, g, deredden != 0, normalise != 0, dz, size, w, c.stream);
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_plan_create(size_t size, double tsamp, const uint64_t* widths, size_t nw, double pmin, double pmax,
                   size_t bmin, size_t bmax, rt_plan** plan)
{
    return guarded([&] {
        ck(hipSetDevice(g_device), "hipSetDevice");
        *plan = make_plan(size, tsamp, widths, nw, pmin, pmax, bmin, bmax);
        return RT_OK;
    });
}

void rt_plan_destroy(rt_plan* plan) { delete plan; }

int rt_plan_shape(const rt_plan* P, size_t* length, size_t* nw)
{
    *length = P->pg.length;
    *nw = P->widths.size();
    return RT_OK;
}

int rt_plan_grid(const rt_plan* P, double* periods, uint32_t* foldbins)
{
    return guarded([&] {
        fill_grid(P->pg, periods, foldbins);
        return RT_OK;
    });
}

int rt_plan_workspace_bytes(const rt_plan* P, size_t batch, size_t* bytes)
{
    *bytes = plan_ws_bytes(P, batch);
    return RT_OK;
}

int rt_periodogram_device(const rt_plan* P, const float* d_data, size_t batch, size_t data_stride, float* d_snrs,
                          size_t snr_stride, void* ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        if (!batch || !P->pg.length) return RT_OK;
        run_periodogram(P, d_data, batch, data_stride, d_snrs, snr_stride, ws, ws_bytes, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_periodogram_ladder_device(const rt_plan* P, const float* d_data, size_t batch, size_t data_stride, void* ws,
                                 size_t ws_bytes, void* stream)
{
    return guarded([&] {
        if (!batch || !P->pg.length) return RT_OK;
        run_ladder(P, d_data, batch, data_stride, ws, ws_bytes, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_periodogram_passes_device(const rt_plan* P, size_t batch, float* d_snrs, size_t snr_stride, void* ws,
                                 size_t ws_bytes, void* stream)
{
    return guarded([&] {
        if (!batch || !P->pg.length) return RT_OK;
        run_passes(P, batch, d_snrs, snr_stride, ws, ws_bytes, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_plan_check(const rt_plan* P, void* stream)
{
    return guarded([&] {
        hipStream_t s = (hipStream_t)stream;
        int flag = 0;
        ck(hipMemcpyAsync(&flag, P->d_flag, sizeof flag, hipMemcpyDeviceToHost, s), "hipMemcpyAsync D2H");
        ck(hipStreamSynchronize(s), "hipStreamSynchronize");
        if (flag) {
            ck(hipMemsetAsync(P->d_flag, 0, sizeof(int), s), "hipMemsetAsync");
            ck(hipStreamSynchronize(s), "hipStreamSynchronize");
            throw std::runtime_error("cone kernel: work item exceeded the LDS budget (S/N rows left unwritten)");
        }
        return RT_OK;
    });
}

int rt_deredden_workspace_bytes(size_t size, size_t ws, size_t minpts, size_t batch, size_t* bytes)
{
    return guarded([&] {
        *bytes = dered_ws_bytes(dered_geom(size, ws, minpts, batch, true));
        return RT_OK;
    });
}

int rt_deredden_normalise_device(const float* d_in, size_t size, size_t batch, size_t in_stride, size_t ws,
                                 size_t minpts, int deredden, int normalise, float* d_out, size_t out_stride,
                                 void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, batch, deredden != 0);
        if (ws_bytes < dered_ws_bytes(g)) throw std::invalid_argument("workspace too small");
        if (deredden && d_in == d_out) throw std::invalid_argument("deredden cannot run in place");
        run_deredden_normalise(d_in, size, batch, in_stride, g, deredden != 0, normalise != 0, d_out, out_stride,
                               d_ws, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_segment_order_stats_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length,
                                  size_t num_widths, size_t nseg, size_t per_seg, const uint32_t* ranks,
                                  size_t nranks, float* d_out, void* stream)
{
    return guarded([&] {
        if (!batch || !num_widths || !nseg) return RT_OK;
        if (per_seg == 0 || nseg * per_seg > length) throw std::invalid_argument("segments exceed the periodogram");
        if (per_seg > (size_t)kMaxSegmentPoints)
            throw std::invalid_argument("segment longer than the device sort (32768 points)");
        if (!nranks || nranks > (size_t)kMaxSegmentRanks) throw std::invalid_argument("1 to 8 ranks per segment");
        for (size_t r = 0; r < nranks; ++r)
            if (ranks[r] >= per_seg) throw std::invalid_argument("rank outside the segment");
        if (batch > 65535 || num_widths > 65535 || nseg > 0x7FFFFFFFull)
            throw std::invalid_argument("segment grid too large");
        ck(launch_segment_order_stats(d_snrs, snr_stride, (uint32_t)batch, (uint32_t)num_widths, (uint32_t)nseg,
                                      (uint32_t)per_seg, ranks, (uint32_t)nranks, d_out, (hipStream_t)stream),
           "segment_order_stats");
        return RT_OK;
    });
}

int rt_threshold_select_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length,
                               size_t num_widths, const double* d_logf, const double* d_coeffs, size_t ncoef,
                               double smin, uint32_t* d_counts, uint32_t* d_idx, size_t cap, void* stream)
{
    return guarded([&] {
        if (!batch || !num_widths) return RT_OK;
        if (!ncoef || ncoef > 64) throw std::invalid_argument("1 to 64 polynomial coefficients");
        if (length > 0xFFFFFFFFull || cap > 0xFFFFFFFFull || batch > 65535 || num_widths > 65535)
            throw std::invalid_argument("threshold selection too large");
        hipStream_t s = (hipStream_t)stream;
        ck(hipMemsetAsync(d_counts, 0, batch * num_widths * sizeof(uint32_t), s), "hipMemsetAsync");
        ck(launch_threshold_select(d_snrs, snr_stride, (uint32_t)batch, (uint32_t)length, (uint32_t)num_widths, d_logf,
                                   d_coeffs, (uint32_t)ncoef, smin, d_counts, d_idx, (uint32_t)cap, s),
           "threshold_select");
        return RT_OK;
    });
}

int rt_find_peaks_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length, size_t num_widths,
                         const double* d_logf, const double* d_freqs, const double* d_coeffs, size_t ncoef,
                         double smin, double radius, uint32_t* d_counts, uint32_t* d_rows, float* d_snr, size_t cap,
                         size_t chunk_rows, void* d_workspace, size_t workspace_bytes, void* stream)
{
    return guarded([&] {
        if (!cap || cap > 0xFFFFFFFFull) throw std::invalid_argument("rt_find_peaks_device: cap must be 1 to 2^32 - 1");
        if (!ncoef || ncoef > 64) throw std::invalid_argument("rt_find_peaks_device: 1 to 64 polynomial coefficients");
        const size_t need = checked_peak_workspace(batch, length, num_widths, chunk_rows);
        if (workspace_bytes < need) throw std::invalid_argument("rt_find_peaks_device: workspace too small");
        if (!batch || !length || !num_widths) {
            // no row: every column has no cluster
            if (batch && num_widths)
                ck(hipMemsetAsync(d_counts, 0, batch * num_widths * sizeof(uint32_t), (hipStream_t)stream),
                   "hipMemsetAsync");
            return RT_OK;
        }
        if ((uintptr_t)d_workspace % 8) throw std::invalid_argument("rt_find_peaks_device: workspace not 8-byte aligned");
        ck(launch_find_peaks(d_snrs, snr_stride, (uint32_t)batch, (uint32_t)length, (uint32_t)num_widths, d_logf,
                             d_freqs, d_coeffs, (uint32_t)ncoef, smin, radius, d_counts, d_rows, d_snr, (uint32_t)cap,
                             peak_chunk_rows(chunk_rows), d_workspace, (hipStream_t)stream),
           "find_peaks");
        return RT_OK;
    });
}

int rt_convert_samples_device(const void* d_raw, size_t n, int is_signed, float* d_out, void* stream)
{
    return guarded([&] {
        if (n >= (1ull << 42)) throw std::invalid_argument("too many samples");
        ck(launch_convert_samples(d_raw, n, is_signed, d_out, (hipStream_t)stream), "convert_samples");
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

int rt_diag_stamps(uint64_t* out8, int reset)
{
    return guarded([&] {
        if (!g_stamps) {
            ck(hipMalloc(&g_stamps, kTimelineCap * kStampRecWords * sizeof(unsigned long long)), "hipMalloc");
            ck(hipMemset(g_stamps, 0, kTimelineCap * kStampRecWords * sizeof(unsigned long long)), "hipMemset");
        }
        ck(hipDeviceSynchronize(), "hipDeviceSynchronize");
        for (int i = 0; i < 8; ++i) out8[i] = 0;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        out8[0] = g_stamp_units;
        if (reset) {
            g_stamp_units = 0;
            g_stamp_launch.clear();
        }
        return RT_OK;
    });
}

int rt_diag_launches(uint64_t* out, uint64_t cap, uint64_t* count)
{
    return guarded([&] {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        const uint64_t n = std::min<uint64_t>(g_stamp_launch.size(), cap);
        for (uint64_t i = 0; i < n; ++i) out[i] = g_stamp_launch[i];
        *count = n;
        return RT_OK;
    });
}

int rt_diag_timeline(uint64_t* out, uint64_t cap, uint64_t* count)
{
    return guarded([&] {
        *count = 0;
        if (!g_stamps) return RT_OK;
        ck(hipDeviceSynchronize(), "hipDeviceSynchronize");
        const uint64_t n = std::min<uint64_t>(std::min<uint64_t>(g_stamp_units, kTimelineCap), cap);
        *count = n;
        if (n)
            ck(hipMemcpy(out, g_stamps, n * kStampRecWords * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy");
        return RT_OK;
    });
}

int rt_plan_stats(const rt_plan* P, uint64_t* transforms, uint64_t* items, uint64_t* launches, double* alg,
                  double* moved, uint64_t* cells)
{
    const ExecTotals t = exec_totals(P->dp.ex);
    *transforms = t.transforms;
    *items = t.items;
    *launches = t.launches;
    *alg = t.alg_bytes;
    *moved = t.moved_bytes;
    *cells = t.cells;
    return RT_OK;
}

}  // extern "C"

#ifdef RT_TEST_HOOKS
int rt_test_corrupt_next_plans(int on)
{
    g_test_corrupt.store(on == 2 ? 2 : (on ? 1 : 0), std::memory_order_relaxed);
    return RT_OK;
}
#endif
