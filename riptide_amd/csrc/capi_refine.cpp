// C ABI, candidate refinement: the pinned staging of the descriptor table and
// the two launches of a plan that refine_host.hpp built and checked.
#include "riptide_amd.h"

#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_device.hpp"
#include "kernels.hpp"
#include "refine_host.hpp"

using namespace rt;

namespace {

std::mutex g_refine_mu;
std::vector<PinnedStage*> g_refine_stages;

void run_refine(const RefinePlan& P, const float* d_cubes, const int32_t* d_shifts, const uint32_t* d_widths,
                float* d_snr, float* d_profiles, void* d_ws, hipStream_t s)
{
    const size_t n = P.cands.size();
    RefineCand* d_cands = (RefineCand*)d_ws;
    float* d_y = (float*)((char*)d_ws + P.table_bytes);
    {
        std::lock_guard<std::mutex> lk(g_refine_mu);
        PinnedStage* st = pinned_stage_acquire(g_refine_stages, n * sizeof(RefineCand));
        std::copy(P.cands.begin(), P.cands.end(), (RefineCand*)st->h);
        ck(hipMemcpyAsync(d_cands, st->h, n * sizeof(RefineCand), hipMemcpyHostToDevice, s), "refine table H2D");
        st->pending = true;
        ck(hipEventRecord(st->ev, s), "hipEventRecord");
    }
    ck(launch_refine(d_cubes, d_shifts, d_widths, d_cands, (uint32_t)n, P.blocks_a, P.blocks_b, P.lds_a, P.lds_b, d_y,
                     d_snr, d_profiles, s),
       "refine");
}

// lengths of the packed host arrays: the furthest end any spec names
struct RefineExtents {
    size_t cubes = 0, shifts = 0, widths = 0, snr = 0, prof = 0;
};

RefineExtents refine_extents(const rt_refine_spec* specs, size_t nspecs)
{
    RefineExtents e;
    for (size_t i = 0; i < nspecs; ++i) {
        const rt_refine_spec& sp = specs[i];
        const size_t B = sp.bands, S = sp.subints, N = sp.bins, K = sp.ndm, J = sp.nper, W = sp.nw;
        e.cubes = std::max(e.cubes, (size_t)sp.cube_off + B * S * N);
        e.shifts = std::max({e.shifts, (size_t)sp.dshift_off + K * B, (size_t)sp.pshift_off + J * S});
        e.widths = std::max(e.widths, (size_t)sp.width_off + W);
        e.snr = std::max(e.snr, (size_t)sp.snr_off + K * J * W);
        e.prof = std::max(e.prof, (size_t)sp.prof_off + K * J * N);
    }
    return e;
}

}  // namespace

extern "C" {

int rt_refine_device(const float* d_cubes, const int32_t* d_shifts, const uint32_t* d_widths,
                     const rt_refine_spec* specs, size_t nspecs, float* d_snr, float* d_profiles, void* d_ws,
                     size_t ws_bytes, void* stream)
{
    return guarded([&] {
        if (!nspecs) return RT_OK;
        const RefinePlan P = refine_plan(specs, nspecs);
        if (ws_bytes < P.ws_bytes) throw std::invalid_argument("workspace too small");
        if (!d_cubes || !d_shifts || !d_widths || !d_snr || !d_ws)
            throw std::invalid_argument("refine: null device pointer");
        run_refine(P, d_cubes, d_shifts, d_widths, d_snr, d_profiles, d_ws, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_refine(const float* cubes, const int32_t* shifts, const uint32_t* widths, const rt_refine_spec* specs,
              size_t nspecs, float* snr, float* profiles)
{
    return guarded([&] {
        if (!nspecs) return RT_OK;
        const RefinePlan P = refine_plan(specs, nspecs);
        if (!cubes || !shifts || !widths || !snr) throw std::invalid_argument("refine: null buffer");
        for (size_t i = 0; i < nspecs; ++i) {
            const rt_refine_spec& sp = specs[i];
            refine_check_tables(sp.bands, sp.subints, sp.bins, shifts + sp.dshift_off, sp.ndm, shifts + sp.pshift_off,
                                sp.nper, widths + sp.width_off, sp.nw, sp.stdnoise);
        }
        const RefineExtents e = refine_extents(specs, nspecs);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, e.cubes);
        int32_t* dsh = dev<int32_t>(c, 1, e.shifts);
        uint32_t* dw = dev<uint32_t>(c, 2, e.widths);
        float* dz = dev<float>(c, 3, e.snr);
        float* dp = profiles ? dev<float>(c, 4, e.prof) : nullptr;
        void* dws = c.buf[5].get(P.ws_bytes);
        h2d(dx, cubes, e.cubes * 4, c.stream);
        h2d(dsh, shifts, e.shifts * 4, c.stream);
        h2d(dw, widths, e.widths * 4, c.stream);
        run_refine(P, dx, dsh, dw, dz, dp, dws, c.stream);
        d2h(snr, dz, e.snr * 4, c.stream);
        if (profiles) d2h(profiles, dp, e.prof * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

}  // extern "C"
