// The host readers of a filterbank block that the host specifications share
// (dedisp_host.cpp, cutout_host.cpp): the one dispatch on the sample type with
// its unpacking, the zero-DM mean series and the block mask's replacement.
// No HIP include.
#pragma once
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "dedisp_types.hpp"

namespace rt {

// The zero-DM mean series (riptide_amd.h, RT_DEDISP_ZERO_DM): Acc = int64_t
// for integer samples (an exact sum), double for float samples.
template <class T>
void zero_dm_mean(const T* x, size_t nsamp, size_t nchans, const uint8_t* mask, float* m)
{
    using Acc = typename std::conditional<std::is_integral<T>::value, int64_t, double>::type;
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

// The replacement of a block mask (riptide_amd.h, rt_block_replace_host): out
// is x with every flagged cell's sample set to its channel's fill, in x's own
// format.  out may be x.
inline void block_replace(const void* x, int dtype, size_t nsamp, size_t nchans, const rt_block_mask* bm, void* out)
{
    const size_t rb = dedisp_row_bytes(dtype, nchans);
    if (out != x) std::memcpy(out, x, nsamp * rb);
    if (!bm) return;
    const int nbits = dedisp_packed_bits(dtype);
    const size_t esize = dedisp_fill_bytes(dtype);
    const uint8_t* fill = (const uint8_t*)bm->fill;
    for (size_t t = 0; t < nsamp; ++t) {
        const uint8_t* flags = bm->cells + (size_t)((bm->t_origin + t) / bm->block_len) * nchans;
        uint8_t* row = (uint8_t*)out + t * rb;
        for (size_t c = 0; c < nchans; ++c) {
            if (!flags[c]) continue;
            if (nbits == 16) {   // the fill is a uint16 of the host, the row little-endian
                uint16_t v;
                std::memcpy(&v, fill + 2 * c, 2);
                row[2 * c] = (uint8_t)(v & 0xFFu);
                row[2 * c + 1] = (uint8_t)(v >> 8);
            } else if (nbits) {   // the low nbits bits of the fill's byte into the channel's field
                const size_t bit = c * (size_t)nbits;
                const unsigned field = (1u << nbits) - 1u, sh = (unsigned)(bit & 7);
                row[bit >> 3] = (uint8_t)((row[bit >> 3] & ~(field << sh)) | ((fill[c] & field) << sh));
            } else {
                std::memcpy(row + c * esize, fill + c * esize, esize);
            }
        }
    }
}

// ---- the sample types (dedisp_types.hpp; riptide_amd.h, RT_DEDISP_U8 .. RT_DEDISP_U16)
// The one unpack helper: channel c of a packed row, as riptide_amd.h defines it.
inline uint32_t unpack_sample(const uint8_t* row, int nbits, size_t c)
{
    if (nbits == 16) return (uint32_t)row[2 * c] | (uint32_t)row[2 * c + 1] << 8;
    const size_t bit = c * (size_t)nbits;
    return (uint32_t)(row[bit >> 3] >> (bit & 7)) & ((1u << nbits) - 1u);
}

// the block as [nsamp, nchans] values: U = uint8_t for 1/2/4 bit, uint16_t for 16 bit
template <class U>
std::vector<U> unpack_block(const void* x, int dtype, size_t nsamp, size_t nchans)
{
    const int nbits = dedisp_packed_bits(dtype);
    const size_t rb = dedisp_row_bytes(dtype, nchans);
    std::vector<U> v(nsamp * nchans);
    for (size_t t = 0; t < nsamp; ++t) {
        const uint8_t* row = (const uint8_t*)x + t * rb;
        for (size_t c = 0; c < nchans; ++c) v[t * nchans + c] = (U)unpack_sample(row, nbits, c);
    }
    return v;
}

// f(the block as a typed [nsamp, nchans] pointer), the one dispatch on the
// sample type: a packed block is unpacked once, 1/2/4 bit to the uint8_t and
// 16 bit to the uint16_t values, and then summed as those
template <class F>
void with_samples(const void* x, int dtype, size_t nsamp, size_t nchans, F f)
{
    if (dedisp_packed_bits(dtype) == 16) f(unpack_block<uint16_t>(x, dtype, nsamp, nchans).data());
    else if (dedisp_packed_bits(dtype)) f(unpack_block<uint8_t>(x, dtype, nsamp, nchans).data());
    else if (dtype == RT_DEDISP_U8) f((const uint8_t*)x);
    else if (dtype == RT_DEDISP_I8) f((const int8_t*)x);
    else f((const float*)x);
}

}  // namespace rt
