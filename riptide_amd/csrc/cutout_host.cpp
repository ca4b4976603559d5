// Pulse cutouts, host side: the sequential specification the kernel of
// cutout_kernels.hip is pinned to (rt_pulse_cutouts_host, riptide_amd.h).  The
// block is read through the readers the dedispersion's specification uses
// (dedisp_host.hpp: the sample types, the block mask's replacement, the
// zero-DM mean).  No HIP header (`make asan` builds this file as is).
#include "riptide_amd.h"

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "capi_common.hpp"
#include "cutout_host.hpp"
#include "dedisp_host.hpp"

using namespace rt;

namespace {

// One job from typed samples x [nsamp, nchans]; m: the zero-DM mean series, or
// nullptr.  Integer samples without m are summed as integers, everything else
// in one float32 accumulator, a rounded addition per sample: channel outer, j
// inner.  Rows outside [0, nsamp) are skipped.
template <class T>
void cutout_job(const T* x, size_t nsamp, size_t nchans, const int32_t* delays, int64_t max_delay,
                const uint8_t* mask, const float* m, const rt_cutout_spec& job, float* out)
{
    constexpr bool kInts = sizeof(T) == 1;
    const int32_t* del = delays + (size_t)job.delay_row * nchans;
    const int64_t f = job.factor, n_rows = (int64_t)nsamp;
    for (int64_t n = 0; n < (int64_t)job.nbins; ++n) {
        int64_t isum = 0;
        float acc = 0.0f;
        for (size_t c = job.band_lo; c < job.band_hi; ++c) {
            if (mask && mask[c]) continue;
            const int64_t d = std::min<int64_t>(std::max<int64_t>(del[c], 0), max_delay);
            const int64_t first = job.start + n * f + d;
            const int64_t lo = std::max<int64_t>(first, 0), hi = std::min<int64_t>(first + f, n_rows);
            for (int64_t t = lo; t < hi; ++t) {
                const T v = x[(size_t)t * nchans + c];
                if (m) {
                    const float y = (float)v - m[t];
                    acc = acc + y;
                } else if (kInts) {
                    isum += (int64_t)v;
                } else {
                    acc = acc + (float)v;
                }
            }
        }
        out[job.out_off + n] = kInts && !m ? (float)(int32_t)isum : acc;
    }
}

}  // namespace

extern "C" {

int rt_pulse_cutouts_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int32_t* delays,
                          size_t ndelay_rows, int64_t max_delay, const uint8_t* mask, const rt_cutout_spec* jobs,
                          size_t njobs, float* out, size_t out_floats, uint32_t flags, const rt_block_mask* bm)
{
    return guarded([&] {
        cutout_check_shape(dtype, nsamp, nchans, ndelay_rows, max_delay, flags);
        dedisp_check_block_mask(bm, nsamp);
        cutout_check_jobs(jobs, njobs, dtype, flags, nchans, ndelay_rows, out_floats);
        if (!njobs) return RT_OK;
        if (!x || !delays || !out) throw std::invalid_argument("pulse_cutouts: null buffer");
        std::vector<uint8_t> replaced;
        if (bm) {   // x' in x's own format
            replaced.resize(nsamp * dedisp_row_bytes(dtype, nchans));
            block_replace(x, dtype, nsamp, nchans, bm, replaced.data());
            x = replaced.data();
        }
        with_samples(x, dtype, nsamp, nchans, [&](const auto* v) {
            std::vector<float> m;
            if (flags & RT_DEDISP_ZERO_DM) {
                m.resize(nsamp);
                zero_dm_mean(v, nsamp, nchans, mask, m.data());
            }
            for (size_t i = 0; i < njobs; ++i)
                cutout_job(v, nsamp, nchans, delays, max_delay, mask, m.empty() ? nullptr : m.data(), jobs[i], out);
        });
        return RT_OK;
    });
}

int rt_pulse_cutouts_plan(size_t esize, int64_t lo, int64_t hi, size_t* tile, size_t* ndw, int* staged)
{
    return guarded([&] {
        if (esize != 1 && esize != 4)
            throw std::invalid_argument("pulse_cutouts_plan: esize must be 1 (8-bit rows) or 4 (float rows)");
        if (lo < 0 || hi <= lo || hi >= 2147483648ll)
            throw std::invalid_argument("pulse_cutouts_plan: the span must be 0 <= lo < hi < 2^31");
        const CutoutSpan sp = cutout_span((uint32_t)esize, (uint32_t)lo, (uint32_t)hi);
        if (tile) *tile = kCutoutTile;
        if (ndw) *ndw = sp.ndw;
        if (staged) *staged = sp.direct ? 0 : 1;
        return RT_OK;
    });
}

}  // extern "C"
