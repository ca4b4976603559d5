// C ABI, single-pulse search: the pinned staging of the width table and the
// launches of a plan that pulse_host.hpp built and checked.
#include "riptide_amd.h"

#include <cmath>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_device.hpp"
#include "pulse_host.hpp"
#include "pulse_kernels.hpp"

using namespace rt;

namespace {

std::mutex g_pulse_mu;
std::vector<PinnedStage*> g_pulse_stages;

}  // namespace

extern "C" {

int rt_single_pulse_device(const float* d_x, size_t nseries, size_t size, size_t ldx, const int32_t* widths,
                           size_t num_widths, float threshold, size_t radius, rt_pulse_event* d_events,
                           size_t capacity, uint64_t* d_count, float* d_best, int32_t* d_kbest, void* d_ws,
                           size_t ws_bytes, void* stream)
{
    return guarded([&] {
        pulse_check_args(size, ldx, widths, num_widths, threshold, radius);
        if (nseries > kPulseMaxSeries) throw std::invalid_argument("single pulse: more than 65535 series in a call");
        if (!d_count) throw std::invalid_argument("single pulse: null event counter");
        if (capacity && !d_events) throw std::invalid_argument("single pulse: null events with a capacity");
        hipStream_t s = (hipStream_t)stream;
        if (!nseries) {
            ck(hipMemsetAsync(d_count, 0, sizeof(uint64_t), s), "hipMemsetAsync");
            return RT_OK;
        }
        if (!d_x || !d_ws) throw std::invalid_argument("single pulse: null device pointer");
        const size_t K = num_widths;
        const PulsePlan P = pulse_plan(nseries, size, K, capacity, (uint32_t)widths[K - 1], (uint32_t)radius);
        if (ws_bytes < P.ws_bytes) throw std::invalid_argument("workspace too small");
        if ((uint64_t)nseries * P.tiles > 0x7FFFFFFFull)
            throw std::invalid_argument("single pulse: too much work for one call");
        char* ws = (char*)d_ws;
        PulseWidth* d_widths = (PulseWidth*)(ws + P.off_widths);
        ck(hipMemsetAsync(ws, 0, 256, s), "hipMemsetAsync");
        {
            std::lock_guard<std::mutex> lk(g_pulse_mu);
            PinnedStage* st = pinned_stage_acquire(g_pulse_stages, K * sizeof(PulseWidth));
            PulseWidth* h = (PulseWidth*)st->h;
            for (size_t k = 0; k < K; ++k) h[k] = PulseWidth{widths[k], widths[k] / 2, std::sqrt((double)widths[k])};
            ck(hipMemcpyAsync(d_widths, h, K * sizeof(PulseWidth), hipMemcpyHostToDevice, s), "pulse widths H2D");
            st->pending = true;
            ck(hipEventRecord(st->ev, s), "hipEventRecord");
        }
        PulseArgs A{};
        A.x = d_x;
        A.ldx = ldx;
        A.N = (uint32_t)size;
        A.K = (uint32_t)K;
        A.widths = d_widths;
        A.threshold = threshold;
        A.R = (uint32_t)radius;
        A.wmax = (uint32_t)widths[K - 1];
        A.tiles = P.tiles;
        A.chunk = P.chunk;
        A.chunk_segs = P.chunk_segs;
        A.best_floats = P.best_floats;
        A.pool = (rt_pulse_event*)(ws + P.off_pool);
        A.cap = capacity;
        A.cursor = (unsigned long long*)ws;
        A.tile_cnt = (uint32_t*)(ws + P.off_cnt);
        A.tile_pos = (uint64_t*)(ws + P.off_pos);
        A.best = d_best;
        A.kbest = d_kbest;
        ck(launch_single_pulse(A, (uint32_t)nseries, P.lds_bytes, (uint64_t*)(ws + P.off_off), d_events, d_count, s),
           "single pulse");
        return RT_OK;
    });
}

}  // extern "C"
