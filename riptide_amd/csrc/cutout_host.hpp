// Pulse cutouts (rt_pulse_cutouts_*, riptide_amd.h): what the host
// specification (cutout_host.cpp), the C ABI (capi_cutout.cpp) and the kernel
// (cutout_kernels.hip) share -- the checks of a call, one text per condition,
// and the kernel's tile and staging rule.  No HIP include (`make asan` builds
// against this header).  The checks throw std::invalid_argument.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "dedisp_types.hpp"
#include "riptide_amd.h"

namespace rt {

// ---- the kernel's shape (pulse_cutout_kernel)
// A workgroup writes kCutoutTile bins of one job from bin t0, a multiple of
// kCutoutTile, a lane per bin.  Per channel it reads the elements
// [first, first + nb * f) of the channel's row that lie in [0, nsamp_blk),
// first = start + t0 * f + delay and nb the tile's bins.  That span, from the
// dword holding its first element, goes through LDS when it fits
// kCutoutSpanDwords, and is read from the row directly otherwise:
//   8-bit rows  staged iff (lo & 3) + (hi - lo) <= 4096 bytes
//   float rows  staged iff hi - lo <= 1024
// with [lo, hi) the clamped span.  A job has one delay per channel, so a
// span has no spread over DMs: which path a channel takes depends on nb * f,
// on how much of the window lies inside the block and, for 8-bit rows, on
// the alignment of its first sample.
constexpr uint32_t kCutoutTile = 256;           // bins of a tile: one per lane
constexpr uint32_t kCutoutChans = 8;            // channels staged per step
constexpr uint32_t kCutoutSpanDwords = 1024;    // staged dwords of a channel (8 x 4 KiB = 32 KiB of LDS)
constexpr uint32_t kCutoutMaxTiles = 65535;     // tiles of a job: the grid's y

struct CutoutSpan {
    uint32_t first;   // first element staged: lo rounded down to a dword
    uint32_t ndw;     // dwords from there to hi
    bool direct;      // more than the LDS span holds
};

// esize: bytes of a row's element, 1 or 4; [lo, hi) a span inside the row, lo < hi
constexpr CutoutSpan cutout_span(uint32_t esize, uint32_t lo, uint32_t hi)
{
    const uint32_t per = 4 / esize;
    const uint32_t e0 = lo & ~(per - 1);
    const uint32_t ndw = (hi - e0 + per - 1) / per;
    return CutoutSpan{e0, ndw, ndw > kCutoutSpanDwords};
}

// the limits of a window's position: start + nbins * factor + a delay stays
// far inside 64 bits
constexpr int64_t kCutoutMaxStart = (int64_t)1 << 40;

// the block and the delay table of a call, host or device
inline void cutout_check_shape(int dtype, size_t nsamp, size_t nchans, size_t ndelay_rows, int64_t max_delay,
                               uint32_t flags)
{
    dedisp_check_flags(flags);
    if (!dedisp_known_dtype(dtype)) throw std::invalid_argument("pulse_cutouts: unknown sample type code");
    if (!nchans || !ndelay_rows)
        throw std::invalid_argument("pulse_cutouts: nchans and the delay table's rows must be at least 1");
    if (!nsamp) throw std::invalid_argument("pulse_cutouts: the block is empty");
    dedisp_check_chan_cap(dtype, nchans);
    if (nchans > 65535ull * 64) throw std::invalid_argument("pulse_cutouts: too many channels");
    if (nsamp >= (1ull << 31)) throw std::invalid_argument("pulse_cutouts: a block must be below 2^31 samples");
    if (ndelay_rows > 0xFFFFFFFFull / nchans)
        throw std::invalid_argument("pulse_cutouts: the delay table overflows 32 bits");
    if (dedisp_packed_bits(dtype) && dedisp_row_bytes(dtype, nchans) > (~0ull >> 1) / nsamp)
        throw std::invalid_argument("pulse_cutouts: the block's bytes overflow a 64-bit offset");
    if (max_delay < 0 || max_delay >= 2147483648ll)
        throw std::invalid_argument("pulse_cutouts: max_delay is outside [0, 2^31)");
}

// the job table, in host memory: every job inside the delay table, its band a
// channel range, its sum exact (integer rows: 8-bit types without the zero-DM
// filter) and its outputs inside out
inline void cutout_check_jobs(const rt_cutout_spec* jobs, size_t njobs, int dtype, uint32_t flags, size_t nchans,
                              size_t ndelay_rows, size_t out_floats)
{
    if (njobs && !jobs) throw std::invalid_argument("pulse_cutouts: jobs is NULL");
    if (njobs > 0x7FFFFFFFull) throw std::invalid_argument("pulse_cutouts: too many jobs for one call");
    const bool ints = !dedisp_float_rows(dtype, flags);
    for (size_t i = 0; i < njobs; ++i) {
        const rt_cutout_spec& j = jobs[i];
        const std::string who = "pulse_cutouts: job " + std::to_string(i);
        if (!j.factor || !j.nbins) throw std::invalid_argument(who + ": factor and nbins must be at least 1");
        if ((uint64_t)j.factor * j.nbins >= (1ull << 31))
            throw std::invalid_argument(who + ": a window of nbins * factor samples must be below 2^31");
        if (j.nbins > (uint64_t)kCutoutMaxTiles * kCutoutTile)
            throw std::invalid_argument(who + ": too many bins");
        if (j.start < -kCutoutMaxStart || j.start > kCutoutMaxStart)
            throw std::invalid_argument(who + ": start is outside [-2^40, 2^40]");
        if (j.delay_row >= ndelay_rows)
            throw std::invalid_argument(who + ": delay_row " + std::to_string(j.delay_row) + " is not below the " +
                                        std::to_string(ndelay_rows) + " rows of the delay table");
        if (j.band_lo > j.band_hi || j.band_hi > nchans)
            throw std::invalid_argument(who + ": band [" + std::to_string(j.band_lo) + ", " +
                                        std::to_string(j.band_hi) + ") is not a channel range lo <= hi <= " +
                                        std::to_string(nchans));
        if (ints && (uint64_t)(j.band_hi - j.band_lo) * j.factor * 255ull >= (1ull << 31))
            throw std::invalid_argument(who + ": (band_hi - band_lo) * factor * 255 must be below 2^31 for an exact "
                                              "8-bit sum");
        if (j.out_off > out_floats || j.nbins > out_floats - j.out_off)
            throw std::invalid_argument(who + ": its bins reach past the " + std::to_string(out_floats) +
                                        " floats of out");
    }
}

}  // namespace rt
