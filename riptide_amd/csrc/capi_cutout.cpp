// C ABI, pulse cutouts: the checks (cutout_host.hpp), the pinned staging of
// the job table, the block's transpose into the dedispersion workspace and the
// one launch for all jobs.  Every refusal happens before anything is queued.
#include "riptide_amd.h"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_dedisp.hpp"
#include "capi_device.hpp"
#include "cutout_host.hpp"
#include "kernels.hpp"

using namespace rt;

namespace {

// pinned staging buffers of the job tables (capi_device.hpp)
std::mutex g_cutout_mu;
std::vector<PinnedStage*> g_cutout_stages;

}  // namespace

extern "C" {

int rt_pulse_cutouts_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                            const int32_t* d_delays, size_t ndelay_rows, int64_t max_delay, const uint8_t* d_mask,
                            const rt_cutout_spec* jobs, size_t njobs, rt_cutout_spec* d_jobs, float* d_out,
                            size_t out_floats, void* d_ws, size_t ws_bytes, void* stream, uint32_t flags,
                            const rt_block_mask* bm)
{
    return guarded([&] {
        cutout_check_shape(dtype, nsamp_blk, nchans, ndelay_rows, max_delay, flags);
        const DeviceCells dc(bm, dtype, nsamp_blk);
        cutout_check_jobs(jobs, njobs, dtype, flags, nchans, ndelay_rows, out_floats);
        if (!njobs) return RT_OK;
        if (!d_block || !d_delays || !d_jobs || !d_out || !d_ws)
            throw std::invalid_argument("pulse_cutouts: null device pointer");
        if ((uintptr_t)d_ws % 16 || (uintptr_t)d_jobs % 8 || (uintptr_t)d_out % 4 || (uintptr_t)d_delays % 4 ||
            (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("pulse_cutouts: misaligned device pointer");
        if (ws_bytes < dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags))
            throw std::invalid_argument("workspace too small");
        uint32_t max_bins = 0;
        for (size_t i = 0; i < njobs; ++i) max_bins = std::max(max_bins, jobs[i].nbins);
        const uint32_t max_tiles = (max_bins + kCutoutTile - 1) / kCutoutTile;
        hipStream_t s = (hipStream_t)stream;
        {
            std::lock_guard<std::mutex> lk(g_cutout_mu);
            PinnedStage* st = pinned_stage_acquire(g_cutout_stages, njobs * sizeof(rt_cutout_spec));
            std::memcpy(st->h, jobs, njobs * sizeof(rt_cutout_spec));
            ck(hipMemcpyAsync(d_jobs, st->h, njobs * sizeof(rt_cutout_spec), hipMemcpyHostToDevice, s),
               "cutout table H2D");
            st->pending = true;
            ck(hipEventRecord(st->ev, s), "hipEventRecord");
        }
        ck(launch_dedisp_rows(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_mask, d_ws, flags, s, dc.get()),
           "pulse_cutouts rows");
        ck(launch_pulse_cutouts(d_ws, dtype, flags, (uint32_t)nsamp_blk, (uint32_t)nchans, d_delays,
                                (uint32_t)ndelay_rows, (uint32_t)max_delay, d_mask, d_jobs, (uint32_t)njobs, max_tiles,
                                d_out, s),
           "pulse_cutouts");
        return RT_OK;
    });
}

}  // extern "C"
