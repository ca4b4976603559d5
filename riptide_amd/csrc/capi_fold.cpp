// C ABI, candidate folding: the pinned staging of the descriptor tables and
// the two launches of a plan that fold_host.hpp built and checked.
#include "riptide_amd.h"

#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_device.hpp"
#include "fold_host.hpp"
#include "kernels.hpp"

using namespace rt;

namespace {

// pinned staging buffers of the descriptor tables (capi_device.hpp)
std::mutex g_fold_mu;
std::vector<PinnedStage*> g_fold_stages;

void run_fold(const FoldPlan& P, const rt_fold_spec* specs, const float* d_data, size_t size, size_t data_stride,
              float* d_out, void* d_ws, hipStream_t s)
{
    const size_t nr = P.rows.size(), ns = P.sub.size();
    FoldCand* d_rows = (FoldCand*)d_ws;
    FoldCand* d_sub = d_rows + nr;
    float* rows_ws = (float*)((char*)d_ws + P.table_bytes);
    {
        std::lock_guard<std::mutex> lk(g_fold_mu);
        PinnedStage* st = pinned_stage_acquire(g_fold_stages, (nr + ns) * sizeof(FoldCand));
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

}  // namespace

extern "C" {

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

}  // extern "C"
