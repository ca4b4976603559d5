// Incoherent dedispersion, host side: the delay table every caller shares and
// the specification the kernels of dedisp_kernels.hip are pinned to
// (rt_dedisperse_host, in the role rt_find_peaks_host and rt_hdiag_host play
// for theirs).  No HIP header (`make asan` builds this file as is).
#include "riptide_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "capi_common.hpp"
#include "dedisp_host.hpp"
#include "dedisp_types.hpp"

using namespace rt;

namespace {

// A band table of the band forms (rt_dedisperse_bands_host): row (d, b) of out
// sums the channels [lo_b, hi_b) alone.  No table (bands == nullptr, the plain
// forms) is the one band [0, nchans).
struct Bands {
    const uint32_t* bands = nullptr;
    size_t nbands = 1;
    size_t lo(size_t b, size_t) const { return bands ? bands[2 * b] : 0; }
    size_t hi(size_t b, size_t nchans) const { return bands ? bands[2 * b + 1] : nchans; }
};

// Acc: int32_t for 8-bit samples (an exact sum), float for float and 16-bit ones
template <class T>
void dedisperse_rows(const T* x, size_t nchans, const int64_t* delays, const uint8_t* mask, size_t ndm, size_t nout,
                     float* out, const Bands& bt)
{
    using Acc = typename std::conditional<sizeof(T) == 1, int32_t, float>::type;
    for (size_t d = 0; d < ndm; ++d) {
        const int64_t* del = delays + d * nchans;
        for (size_t b = 0; b < bt.nbands; ++b) {
            float* o = out + (d * bt.nbands + b) * nout;
            const size_t lo = bt.lo(b, nchans), hi = bt.hi(b, nchans);
            for (size_t t = 0; t < nout; ++t) {
                Acc acc = 0;
                for (size_t c = lo; c < hi; ++c)
                    if (!mask || !mask[c]) acc += (Acc)x[(t + (size_t)del[c]) * nchans + c];
                o[t] = (float)acc;
            }
        }
    }
}

// m is the mean over the unmasked channels of the whole file, whatever the band
template <class T>
void dedisperse_rows_zero_dm(const T* x, size_t nsamp, size_t nchans, const int64_t* delays, const uint8_t* mask,
                             size_t ndm, size_t nout, float* out, const Bands& bt)
{
    std::vector<float> m(nsamp);
    zero_dm_mean(x, nsamp, nchans, mask, m.data());
    for (size_t d = 0; d < ndm; ++d) {
        const int64_t* del = delays + d * nchans;
        for (size_t b = 0; b < bt.nbands; ++b) {
            float* o = out + (d * bt.nbands + b) * nout;
            const size_t lo = bt.lo(b, nchans), hi = bt.hi(b, nchans);
            for (size_t t = 0; t < nout; ++t) {
                float acc = 0.0f;
                for (size_t c = lo; c < hi; ++c) {
                    if (mask && mask[c]) continue;
                    const size_t tt = t + (size_t)del[c];
                    acc += (float)x[tt * nchans + c] - m[tt];
                }
                o[t] = acc;
            }
        }
    }
}

template <class T>
void channel_stats(const T* x, size_t nsamp, size_t nchans, double* acc)
{
    for (size_t t = 0; t < nsamp; ++t)
        for (size_t c = 0; c < nchans; ++c) {
            const double v = (double)x[t * nchans + c];
            acc[c] += v;
            acc[nchans + c] += v * v;
        }
}

// The block statistics (riptide_amd.h, rt_block_stats_host): stats [nblk, 2,
// nchans], per block of block_len rows the sum and the sum of squares, in the
// float64 order the header states -- chunks of kStatsChunk rows from the
// block's first row, four interleaved partial sums per chunk from 0.0 added as
// ((p0 + p1) + p2) + p3, the chunks added in order from 0.0.  Integer samples
// give exact integers in any order.
constexpr size_t kStatsChunk = 2048;

template <class T>
void block_stats(const T* x, size_t nsamp, size_t nchans, size_t block_len, double* stats)
{
    size_t b = 0;
    for (size_t start = 0; start < nsamp; ++b) {
        const size_t stop = block_len > nsamp - start ? nsamp : start + block_len;
        for (size_t c = 0; c < nchans; ++c) {
            double s = 0.0, q = 0.0;
            for (size_t t0 = start; t0 < stop; t0 += kStatsChunk) {
                const size_t t1 = kStatsChunk > stop - t0 ? stop : t0 + kStatsChunk;
                double ps[4] = {0.0, 0.0, 0.0, 0.0}, pq[4] = {0.0, 0.0, 0.0, 0.0};
                for (size_t t = t0; t < t1; ++t) {
                    const double v = (double)x[t * nchans + c];
                    ps[(t - t0) & 3] += v;
                    pq[(t - t0) & 3] += v * v;
                }
                s += ((ps[0] + ps[1]) + ps[2]) + ps[3];
                q += ((pq[0] + pq[1]) + pq[2]) + pq[3];
            }
            stats[(b * 2) * nchans + c] = s;
            stats[(b * 2 + 1) * nchans + c] = q;
        }
        start = stop;
    }
}

// The specification of the plain and the band forms: the checks every form
// shares, then the sums by sample type.  Throws for what they refuse.
void dedisperse_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                     const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out, uint32_t flags,
                     const Bands& bt)
{
    dedisp_check_flags(flags);
    if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    dedisp_check_dtype(dtype, nchans, false);   // the channel cap comes after the lengths, as it always has
    if (max_delay < 0 || max_delay >= 2147483648ll)
        throw std::invalid_argument("dedisperse: max_delay is outside [0, 2^31)");
    if (nout > nsamp || (uint64_t)max_delay > nsamp - nout)
        throw std::invalid_argument("dedisperse: nout + max_delay exceeds the " + std::to_string(nsamp) +
                                    " samples of the input");
    dedisp_check_chan_cap(dtype, nchans);
    for (size_t i = 0; i < ndm * nchans; ++i)
        if (delays[i] < 0 || delays[i] > max_delay)
            throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
    if (!nout || !bt.nbands) return;
    with_samples(x, dtype, nsamp, nchans, [&](const auto* v) {
        if (flags & RT_DEDISP_ZERO_DM) dedisperse_rows_zero_dm(v, nsamp, nchans, delays, mask, ndm, nout, out, bt);
        else dedisperse_rows(v, nchans, delays, mask, ndm, nout, out, bt);
    });
}

// ---- a step of factor f (riptide_amd.h, rt_dedisperse_ds_host): decimation
// first, z [nz, nchans], then the sum of z along the sweep
// integer samples without the zero-DM filter: exact int32 sums (the cap keeps
// them below 2^24), converted once
template <class T>
void decimate_rows_int(const T* x, size_t nchans, size_t f, size_t nz, float* z)
{
    for (size_t u = 0; u < nz; ++u)
        for (size_t c = 0; c < nchans; ++c) {
            int32_t acc = 0;
            for (size_t i = 0; i < f; ++i) acc += (int32_t)x[(u * f + i) * nchans + c];
            z[u * nchans + c] = (float)acc;
        }
}

// everything else: float32 additions from 0.0f in index order; m (NULL: none)
// is the zero-DM mean series
template <class T>
void decimate_rows_f32(const T* x, size_t nchans, size_t f, size_t nz, const float* m, float* z)
{
    for (size_t u = 0; u < nz; ++u)
        for (size_t c = 0; c < nchans; ++c) {
            float acc = 0.0f;
            for (size_t i = 0; i < f; ++i) {
                const size_t t = u * f + i;
                const float v = (float)x[t * nchans + c];
                acc += m ? v - m[t] : v;
            }
            z[u * nchans + c] = acc;
        }
}

void dedisperse_ds_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                        const uint8_t* mask, size_t ndm, int64_t max_delay, size_t f, size_t nout, float* out,
                        uint32_t flags, const rt_block_mask* bm)
{
    dedisp_check_flags(flags);
    if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    dedisp_check_dtype(dtype, nchans, false);
    dedisp_check_downsamp(f);
    dedisp_check_block_mask(bm, nsamp);
    dedisp_check_mask_origin(bm, f);
    std::vector<uint8_t> replaced;
    if (bm && nsamp) {
        if (!x) throw std::invalid_argument("dedisperse: null buffer");
        replaced.resize(nsamp * dedisp_row_bytes(dtype, nchans));
        block_replace(x, dtype, nsamp, nchans, bm, replaced.data());
        x = replaced.data();
    }
    if (f == 1) {   // today's path, today's bits
        dedisperse_host(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, nout, out, flags, Bands{});
        return;
    }
    const size_t nz = nsamp / f;
    if (max_delay < 0 || max_delay >= 2147483648ll)
        throw std::invalid_argument("dedisperse: max_delay is outside [0, 2^31)");
    if (nout > nz || (uint64_t)max_delay > nz - nout)
        throw std::invalid_argument("dedisperse: nout + max_delay exceeds the " + std::to_string(nz) +
                                    " decimated samples of the input");
    dedisp_check_chan_cap(dtype, nchans);
    dedisp_check_ds_cap(dtype, nchans, f, flags);
    for (size_t i = 0; i < ndm * nchans; ++i)
        if (delays[i] < 0 || delays[i] > max_delay)
            throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
    if (!nout) return;
    std::vector<float> z(nz * nchans);
    with_samples(x, dtype, nsamp, nchans, [&](const auto* v) {
        using T = typename std::remove_cv<typename std::remove_pointer<decltype(v)>::type>::type;
        if (flags & RT_DEDISP_ZERO_DM) {
            std::vector<float> m(nsamp);
            zero_dm_mean(v, nsamp, nchans, mask, m.data());
            decimate_rows_f32(v, nchans, f, nz, m.data(), z.data());
        } else if constexpr (sizeof(T) == 1) {
            decimate_rows_int(v, nchans, f, nz, z.data());
        } else {
            decimate_rows_f32(v, nchans, f, nz, (const float*)nullptr, z.data());
        }
    });
    dedisperse_rows(z.data(), nchans, delays, mask, ndm, nout, out, Bands{});   // float32, in channel order
}

// ---- the DM plan (riptide_amd.h, rt_dm_plan)
bool positive(double v) { return v > 0.0 && std::isfinite(v); }

struct DmPlanner {
    double kdisp, ksmear, wmin, step;   // step: tsamp * oversample
    uint32_t max_downsamp;
    double smear(double dm) const { return std::max(wmin, ksmear * dm); }
    double radius(double dm) const { return smear(dm) / kdisp; }
    double next(double dm) const
    {
        const double e = dm + radius(dm);
        const double flat = e + wmin / kdisp;
        return ksmear * flat > wmin ? e / (1.0 - ksmear / kdisp) : flat;
    }
    uint32_t downsamp(double dm) const
    {
        uint32_t f = 1;
        while (2 * f <= max_downsamp && (double)(2 * f) * step <= smear(dm)) f *= 2;
        return f;
    }
};

DmPlanner dm_planner(const double* freqs, size_t nchans, double tsamp, double dm_min, double dm_max, double wmin,
                     double oversample, uint32_t max_downsamp, double kdm)
{
    if (nchans < 2) throw std::invalid_argument("dm_plan: at least 2 channels are needed");
    if (!freqs) throw std::invalid_argument("dm_plan: freqs is NULL");
    double fmin = freqs[0], fmax = freqs[0];
    for (size_t c = 0; c < nchans; ++c) {
        if (!positive(freqs[c]))
            throw std::invalid_argument("dm_plan: channel frequencies must be positive and finite");
        fmin = std::min(fmin, freqs[c]);
        fmax = std::max(fmax, freqs[c]);
    }
    if (!positive(tsamp)) throw std::invalid_argument("dm_plan: tsamp must be positive and finite");
    if (!positive(wmin)) throw std::invalid_argument("dm_plan: wmin must be positive and finite");
    if (!positive(oversample)) throw std::invalid_argument("dm_plan: oversample must be positive and finite");
    if (!positive(kdm)) throw std::invalid_argument("dm_plan: kdm must be positive and finite");
    if (!(dm_min >= 0.0) || !std::isfinite(dm_min))
        throw std::invalid_argument("dm_plan: dm_min must be non-negative and finite");
    if (!(dm_max >= dm_min) || !std::isfinite(dm_max))
        throw std::invalid_argument("dm_plan: dm_max must be finite and at least dm_min");
    if (max_downsamp < 1 || max_downsamp > RT_DEDISP_MAX_DOWNSAMP)
        throw std::invalid_argument("dm_plan: max_downsamp must be in [1, " +
                                    std::to_string(RT_DEDISP_MAX_DOWNSAMP) + "]");
    const double cw = (fmax - fmin) / (double)(nchans - 1);
    const double flo = fmin - cw / 2.0, fhi = fmax + cw / 2.0;
    if (!positive(cw) || !positive(flo))
        throw std::invalid_argument("dm_plan: the channels must span a band above 0 MHz");
    const double fmid = (flo + fhi) / 2.0;
    const double a = fmid - cw / 2.0, b = fmid + cw / 2.0;
    DmPlanner p;
    p.kdisp = kdm * (1.0 / (flo * flo) - 1.0 / (fhi * fhi));
    p.ksmear = kdm * (1.0 / (a * a) - 1.0 / (b * b));
    p.wmin = wmin;
    p.step = tsamp * oversample;
    p.max_downsamp = max_downsamp;
    if (!positive(p.kdisp) || !positive(p.ksmear) || !(p.ksmear < p.kdisp))
        throw std::invalid_argument("dm_plan: the band gives no usable dispersion sweep");
    return p;
}

}  // namespace

extern "C" {

int rt_dm_plan(const double* freqs_mhz, size_t nchans, double tsamp, double dm_min, double dm_max, double wmin,
               double oversample, uint32_t max_downsamp, double kdm, double* dms, uint32_t* downsamp,
               size_t capacity, size_t* ntrials)
{
    return guarded([&] {
        if (!ntrials) throw std::invalid_argument("dm_plan: ntrials is NULL");
        if (!dms != !downsamp) throw std::invalid_argument("dm_plan: dms and downsamp go together");
        const DmPlanner p = dm_planner(freqs_mhz, nchans, tsamp, dm_min, dm_max, wmin, oversample, max_downsamp, kdm);
        size_t n = 0;
        for (double dm = dm_min;; dm = p.next(dm)) {
            if (n >= RT_DM_PLAN_MAX_TRIALS)
                throw std::invalid_argument("dm_plan: more than 2^20 trials: raise wmin or lower dm_max");
            if (dms) {
                if (n >= capacity) throw std::invalid_argument("dm_plan: capacity is below the number of trials");
                dms[n] = dm;
                downsamp[n] = p.downsamp(dm);
            }
            ++n;
            if (dm + p.radius(dm) >= dm_max) break;
        }
        *ntrials = n;
        return RT_OK;
    });
}

int rt_dedisperse_ds_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                          const uint8_t* mask, size_t ndm, int64_t max_delay, size_t downsamp, size_t nout,
                          float* out, uint32_t flags, const rt_block_mask* bm)
{
    return guarded([&] {
        dedisperse_ds_host(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, downsamp, nout, out, flags, bm);
        return RT_OK;
    });
}

int rt_dedisperse_steps_check(int dtype, size_t nsamp_blk, size_t nchans, const rt_dedisp_step* steps,
                              size_t nsteps, size_t delays_len, size_t out_floats, uint32_t flags,
                              const rt_block_mask* bm)
{
    return guarded([&] {
        dedisp_check_steps(dtype, nsamp_blk, nchans, steps, nsteps, delays_len, out_floats, flags, bm);
        return RT_OK;
    });
}

int rt_dedisp_row_bytes(int dtype, size_t nchans, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("dedisperse: bytes is NULL");
        dedisp_check_dtype(dtype, nchans, false);
        *bytes = dedisp_row_bytes(dtype, nchans);
        return RT_OK;
    });
}

int rt_dedisperse_delays(const double* freqs_mhz, size_t nchans, const double* dms, size_t ndm, double tsamp,
                         double kdm, int64_t* delays, int64_t* max_delay)
{
    return guarded([&] {
        if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
        if (!(tsamp > 0.0) || !std::isfinite(tsamp)) throw std::invalid_argument("dedisperse: tsamp must be > 0");
        if (!std::isfinite(kdm)) throw std::invalid_argument("dedisperse: kdm must be finite");
        double f_ref = 0.0;
        for (size_t c = 0; c < nchans; ++c) {
            const double f = freqs_mhz[c];
            if (!(f > 0.0) || !std::isfinite(f))
                throw std::invalid_argument("dedisperse: channel frequencies must be positive and finite");
            if (f > f_ref) f_ref = f;
        }
        for (size_t d = 0; d < ndm; ++d)
            if (!(dms[d] >= 0.0) || !std::isfinite(dms[d]))
                throw std::invalid_argument("dedisperse: DMs must be non-negative and finite");
        int64_t dmax = 0;
        for (size_t d = 0; d < ndm; ++d)
            for (size_t c = 0; c < nchans; ++c) {
                const double f = freqs_mhz[c];
                const double a = 1.0 / (f * f) - 1.0 / (f_ref * f_ref);
                const double v = std::floor(kdm * dms[d] * a / tsamp + 0.5);
                if (!(v < 2147483648.0) || !(v >= 0.0))
                    throw std::invalid_argument("dedisperse: a delay is outside [0, 2^31) samples");
                const int64_t k = (int64_t)v;
                delays[d * nchans + c] = k;
                if (k > dmax) dmax = k;
            }
        if (max_delay) *max_delay = dmax;
        return RT_OK;
    });
}

int rt_dedisperse_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                       const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out)
{
    return rt_dedisperse_host_opt(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, nout, out, 0u);
}

int rt_dedisperse_host_opt(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                           const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out,
                           uint32_t flags)
{
    return guarded([&] {
        dedisperse_host(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, nout, out, flags, Bands{});
        return RT_OK;
    });
}

int rt_dedisperse_bands_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                             const uint8_t* mask, size_t ndm, const uint32_t* bands, size_t nbands,
                             int64_t max_delay, size_t nout, float* out, uint32_t flags)
{
    return guarded([&] {
        if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
        if (nbands && !bands) throw std::invalid_argument("dedisperse: bands is NULL");
        dedisp_check_band_table(bands, nbands, nchans);
        dedisperse_host(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, nout, out, flags, Bands{bands, nbands});
        return RT_OK;
    });
}

int rt_dedisperse_span_plan(size_t esize, int64_t lo, int64_t hi, size_t* ndw, int* staged)
{
    return guarded([&] {
        if (esize != 1 && esize != 4)
            throw std::invalid_argument("span_plan: esize must be 1 (8-bit rows) or 4 (float rows)");
        if (lo < 0 || hi < lo || hi >= 2147483648ll)
            throw std::invalid_argument("span_plan: the delays must be 0 <= lo <= hi < 2^31");
        const DedispSpan sp = dedisp_span((uint32_t)esize, (uint32_t)lo, (uint32_t)hi);
        if (ndw) *ndw = sp.ndw;
        if (staged) *staged = sp.direct ? 0 : 1;
        return RT_OK;
    });
}

int rt_zero_dm_mean_host(const void* x, int dtype, size_t nsamp, size_t nchans, const uint8_t* mask, float* m)
{
    return guarded([&] {
        dedisp_check_dtype(dtype, nchans, true);
        if (!nsamp) return RT_OK;
        if (!x || !m) throw std::invalid_argument("zero_dm_mean: null buffer");
        with_samples(x, dtype, nsamp, nchans, [&](const auto* v) { zero_dm_mean(v, nsamp, nchans, mask, m); });
        return RT_OK;
    });
}

int rt_channel_stats_host(const void* x, int dtype, size_t nsamp, size_t nchans, double* acc)
{
    return guarded([&] {
        dedisp_check_dtype(dtype, nchans, false, "channel_stats");   // the statistics have no channel cap
        if (!acc) throw std::invalid_argument("channel_stats: null buffer");
        if (!nsamp) return RT_OK;
        if (!x) throw std::invalid_argument("channel_stats: null buffer");
        with_samples(x, dtype, nsamp, nchans, [&](const auto* v) { channel_stats(v, nsamp, nchans, acc); });
        return RT_OK;
    });
}

int rt_block_replace_host(const void* x, int dtype, size_t nsamp, size_t nchans, const rt_block_mask* bm, void* out)
{
    return guarded([&] {
        dedisp_check_dtype(dtype, nchans, false, "block_mask");
        dedisp_check_block_mask(bm, nsamp);
        if (!nsamp) return RT_OK;
        if (!x || !out) throw std::invalid_argument("block_mask: null buffer");
        block_replace(x, dtype, nsamp, nchans, bm, out);
        return RT_OK;
    });
}

int rt_block_stats_host(const void* x, int dtype, size_t nsamp, size_t nchans, size_t block_len, double* stats)
{
    return guarded([&] {
        dedisp_check_dtype(dtype, nchans, false, "block_stats");   // the statistics have no channel cap
        if (!block_len) throw std::invalid_argument("block_stats: block_len must be at least 1");
        if (!nsamp) return RT_OK;
        if (!x || !stats) throw std::invalid_argument("block_stats: null buffer");
        with_samples(x, dtype, nsamp, nchans, [&](const auto* v) { block_stats(v, nsamp, nchans, block_len, stats); });
        return RT_OK;
    });
}

}  // extern "C"
