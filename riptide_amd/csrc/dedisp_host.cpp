// Incoherent dedispersion, host side: the delay table every caller shares and
// the specification the kernels of dedisp_kernels.hip are pinned to
// (rt_dedisperse_host, in the role rt_find_peaks_host and rt_hdiag_host play
// for theirs).  No HIP header (`make asan` builds this file as is).
#include "riptide_amd.h"

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "capi_common.hpp"

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

template <class T, class Acc>
void dedisperse_rows(const T* x, size_t nchans, const int64_t* delays, const uint8_t* mask, size_t ndm, size_t nout,
                     float* out, const Bands& bt)
{
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

// The zero-DM mean series (riptide_amd.h, RT_DEDISP_ZERO_DM): Acc = int64_t
// for 8-bit samples (an exact sum), double for float samples.
template <class T, class Acc>
void zero_dm_mean(const T* x, size_t nsamp, size_t nchans, const uint8_t* mask, float* m)
{
    size_t nu = 0;
    for (size_t c = 0; c < nchans; ++c) nu += !mask || !mask[c];
    for (size_t t = 0; t < nsamp; ++t) {
        Acc s = 0;
        const T* row = x + t * nchans;
        for (size_t c = 0; c < nchans; ++c)
            if (!mask || !mask[c]) s += (Acc)row[c];
        m[t] = nu ? (float)((double)s / (double)nu) : 0.0f;
    }
}

// m is the mean over the unmasked channels of the whole file, whatever the band
template <class T>
void dedisperse_rows_zero_dm(const T* x, size_t nsamp, size_t nchans, const int64_t* delays, const uint8_t* mask,
                             size_t ndm, size_t nout, float* out, const Bands& bt)
{
    std::vector<float> m(nsamp);
    zero_dm_mean<T, typename std::conditional<std::is_integral<T>::value, int64_t, double>::type>(x, nsamp, nchans,
                                                                                                  mask, m.data());
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

// ---- packed sample types (riptide_amd.h, RT_DEDISP_U1 .. RT_DEDISP_U16)
// bits of a packed code, 0 for any other
int packed_bits(int dtype)
{
    return dtype == RT_DEDISP_U1 ? 1 : dtype == RT_DEDISP_U2 ? 2 : dtype == RT_DEDISP_U4 ? 4
           : dtype == RT_DEDISP_U16 ? 16 : 0;
}

bool known_dtype(int dtype)
{
    return dtype == RT_DEDISP_U8 || dtype == RT_DEDISP_I8 || dtype == RT_DEDISP_F32 || packed_bits(dtype);
}

// summed as integers, exact in float32 up to RT_DEDISP_MAX_CHANS_8BIT channels
bool integer_sum(int dtype) { return dtype != RT_DEDISP_F32 && dtype != RT_DEDISP_U16; }

// The one unpack helper: channel c of a packed row, as riptide_amd.h defines it.
inline uint32_t unpack_sample(const uint8_t* row, int nbits, size_t c)
{
    if (nbits == 16) return (uint32_t)row[2 * c] | (uint32_t)row[2 * c + 1] << 8;
    const size_t bit = c * (size_t)nbits;
    return (uint32_t)(row[bit >> 3] >> (bit & 7)) & ((1u << nbits) - 1u);
}

size_t packed_row_bytes(int nbits, size_t nchans)
{
    if (nchans > SIZE_MAX / 16 || nchans * (size_t)nbits % 8)
        throw std::invalid_argument("dedisperse: " + std::to_string(nchans) + " channels of " + std::to_string(nbits) +
                                    "-bit data: rows are not a whole number of bytes");
    return nchans * (size_t)nbits / 8;
}

// the block as [nsamp, nchans] values: U = uint8_t for 1/2/4 bit, uint16_t for 16 bit
template <class U>
std::vector<U> unpack_block(const void* x, int nbits, size_t nsamp, size_t nchans)
{
    const size_t rb = packed_row_bytes(nbits, nchans);
    std::vector<U> v(nsamp * nchans);
    for (size_t t = 0; t < nsamp; ++t) {
        const uint8_t* row = (const uint8_t*)x + t * rb;
        for (size_t c = 0; c < nchans; ++c) v[t * nchans + c] = (U)unpack_sample(row, nbits, c);
    }
    return v;
}

void check_dtype(int dtype, size_t nchans)
{
    if (!known_dtype(dtype)) throw std::invalid_argument("dedisperse: unknown sample type code");
    if (!nchans) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    if (integer_sum(dtype) && nchans > RT_DEDISP_MAX_CHANS_8BIT)
        throw std::invalid_argument("dedisperse: too many channels for an exact 8-bit sum");
    if (packed_bits(dtype)) packed_row_bytes(packed_bits(dtype), nchans);
}

// The specification of the plain and the band forms: the checks every form
// shares, then the sums by sample type.  Throws for what they refuse.
void dedisperse_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                     const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out, uint32_t flags,
                     const Bands& bt)
{
    if (flags & ~RT_DEDISP_ZERO_DM) throw std::invalid_argument("dedisperse: unknown flag bit");
    if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    if (!known_dtype(dtype)) throw std::invalid_argument("dedisperse: unknown sample type code");
    const int nbits = packed_bits(dtype);
    if (nbits) packed_row_bytes(nbits, nchans);
    if (max_delay < 0 || max_delay >= 2147483648ll)
        throw std::invalid_argument("dedisperse: max_delay is outside [0, 2^31)");
    if (nout > nsamp || (uint64_t)max_delay > nsamp - nout)
        throw std::invalid_argument("dedisperse: nout + max_delay exceeds the " + std::to_string(nsamp) +
                                    " samples of the input");
    if (integer_sum(dtype) && nchans > RT_DEDISP_MAX_CHANS_8BIT)
        throw std::invalid_argument("dedisperse: too many channels for an exact 8-bit sum");
    for (size_t i = 0; i < ndm * nchans; ++i)
        if (delays[i] < 0 || delays[i] > max_delay)
            throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
    if (!nout || !bt.nbands) return;
    if (nbits) {
        // the values of the packed block, then the same sums: 1/2/4 bit as
        // 8-bit data, 16 bit converted exactly and added in float32
        if (nbits == 16) {
            const std::vector<uint16_t> v = unpack_block<uint16_t>(x, nbits, nsamp, nchans);
            if (flags & RT_DEDISP_ZERO_DM)
                dedisperse_rows_zero_dm(v.data(), nsamp, nchans, delays, mask, ndm, nout, out, bt);
            else
                dedisperse_rows<uint16_t, float>(v.data(), nchans, delays, mask, ndm, nout, out, bt);
        } else {
            const std::vector<uint8_t> v = unpack_block<uint8_t>(x, nbits, nsamp, nchans);
            if (flags & RT_DEDISP_ZERO_DM)
                dedisperse_rows_zero_dm(v.data(), nsamp, nchans, delays, mask, ndm, nout, out, bt);
            else
                dedisperse_rows<uint8_t, int32_t>(v.data(), nchans, delays, mask, ndm, nout, out, bt);
        }
        return;
    }
    if (flags & RT_DEDISP_ZERO_DM) {
        if (dtype == RT_DEDISP_U8)
            dedisperse_rows_zero_dm((const uint8_t*)x, nsamp, nchans, delays, mask, ndm, nout, out, bt);
        else if (dtype == RT_DEDISP_I8)
            dedisperse_rows_zero_dm((const int8_t*)x, nsamp, nchans, delays, mask, ndm, nout, out, bt);
        else
            dedisperse_rows_zero_dm((const float*)x, nsamp, nchans, delays, mask, ndm, nout, out, bt);
        return;
    }
    if (dtype == RT_DEDISP_U8)
        dedisperse_rows<uint8_t, int32_t>((const uint8_t*)x, nchans, delays, mask, ndm, nout, out, bt);
    else if (dtype == RT_DEDISP_I8)
        dedisperse_rows<int8_t, int32_t>((const int8_t*)x, nchans, delays, mask, ndm, nout, out, bt);
    else
        dedisperse_rows<float, float>((const float*)x, nchans, delays, mask, ndm, nout, out, bt);
}

}  // namespace

extern "C" {

int rt_dedisp_row_bytes(int dtype, size_t nchans, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("dedisperse: bytes is NULL");
        if (!known_dtype(dtype)) throw std::invalid_argument("dedisperse: unknown sample type code");
        if (!nchans) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
        if (packed_bits(dtype)) {
            *bytes = packed_row_bytes(packed_bits(dtype), nchans);
        } else {
            const size_t esize = dtype == RT_DEDISP_F32 ? 4 : 1;
            if (nchans > SIZE_MAX / esize) throw std::invalid_argument("dedisperse: too many channels");
            *bytes = nchans * esize;
        }
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
        for (size_t b = 0; b < nbands; ++b)
            if (bands[2 * b] > bands[2 * b + 1] || bands[2 * b + 1] > nchans)
                throw std::invalid_argument("dedisperse: band " + std::to_string(b) + " [" +
                                            std::to_string(bands[2 * b]) + ", " + std::to_string(bands[2 * b + 1]) +
                                            ") is not a channel range lo <= hi <= " + std::to_string(nchans));
        dedisperse_host(x, dtype, nsamp, nchans, delays, mask, ndm, max_delay, nout, out, flags, Bands{bands, nbands});
        return RT_OK;
    });
}

int rt_zero_dm_mean_host(const void* x, int dtype, size_t nsamp, size_t nchans, const uint8_t* mask, float* m)
{
    return guarded([&] {
        check_dtype(dtype, nchans);
        if (!nsamp) return RT_OK;
        if (!x || !m) throw std::invalid_argument("zero_dm_mean: null buffer");
        if (packed_bits(dtype) == 16)
            zero_dm_mean<uint16_t, int64_t>(unpack_block<uint16_t>(x, 16, nsamp, nchans).data(), nsamp, nchans, mask, m);
        else if (packed_bits(dtype))
            zero_dm_mean<uint8_t, int64_t>(unpack_block<uint8_t>(x, packed_bits(dtype), nsamp, nchans).data(), nsamp,
                                           nchans, mask, m);
        else if (dtype == RT_DEDISP_U8)
            zero_dm_mean<uint8_t, int64_t>((const uint8_t*)x, nsamp, nchans, mask, m);
        else if (dtype == RT_DEDISP_I8)
            zero_dm_mean<int8_t, int64_t>((const int8_t*)x, nsamp, nchans, mask, m);
        else
            zero_dm_mean<float, double>((const float*)x, nsamp, nchans, mask, m);
        return RT_OK;
    });
}

int rt_channel_stats_host(const void* x, int dtype, size_t nsamp, size_t nchans, double* acc)
{
    return guarded([&] {
        if (!known_dtype(dtype)) throw std::invalid_argument("channel_stats: unknown sample type code");
        if (!nchans) throw std::invalid_argument("channel_stats: nchans must be at least 1");
        if (packed_bits(dtype)) packed_row_bytes(packed_bits(dtype), nchans);
        if (!acc) throw std::invalid_argument("channel_stats: null buffer");
        if (!nsamp) return RT_OK;
        if (!x) throw std::invalid_argument("channel_stats: null buffer");
        if (packed_bits(dtype) == 16)
            channel_stats(unpack_block<uint16_t>(x, 16, nsamp, nchans).data(), nsamp, nchans, acc);
        else if (packed_bits(dtype))
            channel_stats(unpack_block<uint8_t>(x, packed_bits(dtype), nsamp, nchans).data(), nsamp, nchans, acc);
        else if (dtype == RT_DEDISP_U8)
            channel_stats((const uint8_t*)x, nsamp, nchans, acc);
        else if (dtype == RT_DEDISP_I8)
            channel_stats((const int8_t*)x, nsamp, nchans, acc);
        else
            channel_stats((const float*)x, nsamp, nchans, acc);
        return RT_OK;
    });
}

}  // extern "C"
