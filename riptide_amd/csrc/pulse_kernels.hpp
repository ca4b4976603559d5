// Launch wrapper of pulse_kernels.hip (host-callable, stream-ordered, no sync).
#pragma once
#include <hip/hip_runtime.h>

#include "pulse_host.hpp"

namespace rt {

struct PulseArgs {
    const float* x;             // [nseries] rows, ldx floats apart
    uint64_t ldx;
    uint32_t N, K;
    const PulseWidth* widths;   // device table, ascending
    float threshold;
    uint32_t R, wmax;           // radius, largest width
    uint32_t tiles;             // per row
    uint32_t chunk, chunk_segs, best_floats;   // PulsePlan's
    rt_pulse_event* pool;       // cap records, in the order the tiles claimed them
    uint64_t cap;
    unsigned long long* cursor; // the pool's fill, zero before the launch
    uint32_t* tile_cnt;         // [nseries * tiles] events of a tile
    uint64_t* tile_pos;         // its run in the pool
    float* best;                // dense outputs, or null
    int32_t* kbest;
};

// The three launches of a call (pulse_kernels.hip).  The arguments are a
// checked plan's (pulse_plan, pulse_check_args); tile_off: nseries * tiles
// uint64 of workspace.  *d_count: the number of events found.
hipError_t launch_single_pulse(const PulseArgs& A, uint32_t nseries, uint32_t lds_bytes, uint64_t* tile_off,
                               rt_pulse_event* d_events, uint64_t* d_count, hipStream_t s);

}  // namespace rt
