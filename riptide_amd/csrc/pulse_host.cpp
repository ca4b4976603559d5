// C ABI, host-only entry points of the single-pulse search: the specification
// (pulse_host.hpp), the device form's limits and workspace.  No HIP header:
// this file is also built by g++ with the sanitizers (Makefile asan).
#include "riptide_amd.h"

#include <stdexcept>

#include "capi_common.hpp"
#include "pulse_host.hpp"

using namespace rt;

extern "C" {

int rt_single_pulse_host(const float* x, size_t nseries, size_t size, size_t ldx, const int32_t* widths,
                         size_t num_widths, float threshold, size_t radius, rt_pulse_event* events, size_t capacity,
                         uint64_t* count, float* best, int32_t* kbest)
{
    return guarded([&] {
        const uint64_t found = single_pulse_host(x, nseries, size, ldx, widths, num_widths, threshold, radius, events,
                                                 capacity, best, kbest);
        if (count) *count = found;
        return RT_OK;
    });
}

int rt_single_pulse_limits(size_t* tile, size_t* max_width)
{
    if (tile) *tile = kPulseTile;
    if (max_width) *max_width = kPulseMaxWidth;
    return RT_OK;
}

int rt_single_pulse_plan(size_t wmax, size_t radius, size_t* chunk, size_t* chunk_segs, size_t* lds_bytes)
{
    return guarded([&] {
        if (wmax < 1 || wmax > kPulseMaxWidth)
            throw std::invalid_argument("single pulse: the largest width must be in [1, RT_PULSE_MAX_WIDTH]");
        if (radius > kPulseMaxWidth) throw std::invalid_argument("single pulse: radius above RT_PULSE_MAX_WIDTH (6144)");
        const PulsePlan P = pulse_plan(0, 0, 0, 0, (uint32_t)wmax, (uint32_t)radius);
        if (chunk) *chunk = P.chunk;
        if (chunk_segs) *chunk_segs = P.chunk_segs;
        if (lds_bytes) *lds_bytes = P.lds_bytes;
        return RT_OK;
    });
}

int rt_single_pulse_workspace_bytes(size_t nseries, size_t size, size_t num_widths, size_t capacity, size_t* bytes)
{
    return guarded([&] {
        if (!num_widths) throw std::invalid_argument("single pulse: no trial widths");
        if (size > kPulseMaxSamples) throw std::invalid_argument("single pulse: more than 2^30 samples");
        if (nseries > kPulseMaxSeries) throw std::invalid_argument("single pulse: more than 65535 series in a call");
        const size_t need = pulse_plan(nseries, size, num_widths, capacity, 1, 0).ws_bytes;
        if (bytes) *bytes = need;
        return RT_OK;
    });
}

}  // extern "C"
