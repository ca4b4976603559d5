// C ABI, periodogram side: the cone scheduler (a compiled plan resident on a
// device, its launches on one or two streams), rt_plan and the ladder /
// passes drivers, the single-transform FFA, the plan and diagnostic entry
// points.  The test build swaps this one object (RT_TEST_HOOKS).
#include "riptide_amd.h"
#ifdef RT_TEST_HOOKS
#include "riptide_amd_test.h"
#endif

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_device.hpp"
#include "kernels.hpp"
#include "plan.hpp"

using namespace rt;

namespace {

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

// One cone launch of a plan on stream s (profiling: one record around it
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
    ProfScope prof(s, 0, g_prof.on && prof_each);
    prof.add(L.alg_bytes * batch, L.moved_bytes * batch);
    ck(launch_cone(a, L.smax, L.wide_snr != 0, L.snr, s), "cone_kernel");
    prof.finish();
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

// Slot-width buckets on two streams (2 G events): within a transform group
// the launches of different slot widths belong to disjoint transforms
// (independent pass chains), so the group's main bucket (most cells) runs on
// s and the others on a side stream, joined at the group's end (the next
// group reuses the scratch buffers).  Each chain's launch drains fill with the
// other's units: cone ms per trial cfg2 7.092 -> 7.072, cfg3 1.795 -> 1.776,
// cfg1 0.274 -> 0.260 (profiles/r04r_ab_*_bucketstreams.log).  Returns the
// launches issued.
size_t launch_buckets(const DevicePlan& P, const ConeArgs& a, uint32_t batch, hipStream_t s, SideLease& lease,
                      uint32_t G)
{
    const std::vector<Launch>& Ls = P.ex.launches;
    SideSet* const ss = lease.ss;
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
    return li;
}

// Transform groups co-scheduled on two streams (2 + G events): group g on
// stream g mod 2, its merge-only launches starting once group g - 1 has
// finished its own merge-only launches -- so group g's merge-only passes
// (latency / LDS bound) share the CUs with group g - 1's final passes (VALU
// bound: the fused S/N).  Returns the launches issued.
size_t launch_groups(const DevicePlan& P, const ConeArgs& a, uint32_t batch, hipStream_t s, SideLease& lease,
                     uint32_t G)
{
    const std::vector<Launch>& Ls = P.ex.launches;
    SideSet* const ss = lease.ss;
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
    ck(hipEventRecord(join, ss->s2), "hipEventRecord");
    ck(hipStreamWaitEvent(s, join, 0), "hipStreamWaitEvent");
    lease.forked = false;
    return li;
}

// Run all cone launches of an exec plan: on the caller's stream, one
// profiling record per launch, or -- a plan with launches of several slot
// widths, or with two scratch banks (ExecPlan::banks) -- on two streams
// (launch_buckets / launch_groups).  Profiling then records one event pair
// from the fork to the join (launches overlap) with their summed bytes.
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
    const bool buckets = single || P.ex.banks < 2 || P.ex.groups < 2;
    if (buckets) {
        bool multi = false;
        for (const Launch& L : Ls) multi = multi || L.smax != Ls.front().smax;
        if (!multi || single) {
            for (const Launch& L : Ls) cone_launch(P, L, a, batch, s, true);
            return;
        }
    }
    const uint32_t G = buckets ? std::max<uint32_t>(P.ex.groups, 1) : P.ex.groups;
    SideLease lease(P, buckets ? 2 * (size_t)G : 2 + (size_t)G, s);
    ProfScope prof(s, 0, g_prof.on);
    if (prof.on())
        for (const Launch& L : Ls) prof.add(L.alg_bytes * batch, L.moved_bytes * batch);
    const size_t issued = buckets ? launch_buckets(P, a, batch, s, lease, G) : launch_groups(P, a, batch, s, lease, G);
    if (issued != Ls.size()) throw std::runtime_error("cone launches out of group order");
    prof.finish();
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

// The end of a host-buffer call: copies the cone kernel's error flag back
// behind whatever the call has queued on s, waits for it all, and throws if a
// unit set the flag.
void sync_and_check_flag(const int* d_flag, hipStream_t s)
{
    int hflag = 0;
    d2h(&hflag, d_flag, sizeof hflag, s);
    sync(s);
    if (hflag) throw std::runtime_error("cone kernel: work item exceeded the LDS budget");
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
    ProfScope prof(s, 1, g_prof.on);
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
    if (prof.on()) {
        // fused: the series is read once for its rungs; per-rung: once per rung
        double bytes = l.mode != kLadderPerRung ? 4.0 * P->pg.prm.size : 0.0;
        for (const DsRung& d : l.rungs) {
            const bool fused = rung_in_fused(l.mode, d);
            bytes += 4.0 * (double)d.n + (fused ? 0.0 : (d.identity ? 4.0 * d.n : 4.0 * P->pg.prm.size));
        }
        prof.add(bytes * batch, bytes * batch);
        prof.finish();
    }
}

// The FFA passes + fused S/N of a batch whose leaf buffer run_ladder filled.
void run_passes(const rt_plan* P, size_t batch, float* d_snrs, size_t snr_stride, void* ws, size_t ws_bytes,
                hipStream_t s)
{
    const PlanWs W = plan_ws(P, batch, ws, ws_bytes);
    ConeArgs a{};
    a.num_widths = (uint32_t)P->widths.size();
    a.widths = P->d_widths;
    a.leaves = W.leaves;
    a.leaves_stride = P->pg.leaf_floats;
    a.ping = W.ping;
    a.pong = W.pong;
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

}  // namespace

// ---------------------------------------------------------------------------
// entry points
// ---------------------------------------------------------------------------
extern "C" {

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
        d2h(out, dz, n * 4, c.stream);
        sync_and_check_flag(flag, c.stream);
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
        sync_and_check_flag(flag, c.stream);
        *seconds = ms * 1e-3 / (double)loops;
        return RT_OK;
    });
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
        d2h(snrs, dz, L * nw * 4, c.stream);
        sync_and_check_flag(P->d_flag, c.stream);
        return RT_OK;
    });
}

int rt_plan_create(size_t size, double tsamp, const uint64_t* widths, size_t nw, double pmin, double pmax,
                   size_t bmin, size_t bmax, rt_plan** plan)
{
    return guarded([&] {
        ck(hipSetDevice(current_device()), "hipSetDevice");
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

}  // extern "C"

#ifdef RT_TEST_HOOKS
int rt_test_corrupt_next_plans(int on)
{
    g_test_corrupt.store(on == 2 ? 2 : (on ? 1 : 0), std::memory_order_relaxed);
    return RT_OK;
}
#endif
