// The filterbank side's sample types (RT_DEDISP_* of riptide_amd.h) and the
// checks its host specification (dedisp_host.cpp), its C ABI (capi_dedisp.cpp)
// and its launchers (dedisp_kernels.hip) share: one text per condition.  No
// HIP include (`make asan` builds against this header).  The checks throw
// std::invalid_argument, which guarded() turns into RT_EINVAL.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "riptide_amd.h"

namespace rt {

// bits of a packed sample type code (RT_DEDISP_U1, U2, U4, U16: the block is
// then bytes, [nsamp, nchans * bits / 8], byte-aligned), 0 for any other
constexpr int dedisp_packed_bits(int dtype)
{
    return dtype == RT_DEDISP_U1 ? 1 : dtype == RT_DEDISP_U2 ? 2 : dtype == RT_DEDISP_U4 ? 4
           : dtype == RT_DEDISP_U16 ? 16 : 0;
}

constexpr bool dedisp_known_dtype(int dtype)
{
    return dtype == RT_DEDISP_U8 || dtype == RT_DEDISP_I8 || dtype == RT_DEDISP_F32 || dedisp_packed_bits(dtype);
}

// float and 16-bit data are summed in float32; everything else as integers,
// exact in float32 up to RT_DEDISP_MAX_CHANS_8BIT channels
constexpr bool dedisp_integer_sum(int dtype) { return dtype != RT_DEDISP_F32 && dtype != RT_DEDISP_U16; }

// bytes of a row of the block of a known type (rt_dedisp_row_bytes); packed
// rows must be whole bytes
inline size_t dedisp_row_bytes(int dtype, size_t nchans)
{
    const size_t nbits = (size_t)dedisp_packed_bits(dtype);
    if (nbits) {
        if (nchans > SIZE_MAX / 16 || nchans * nbits % 8)
            throw std::invalid_argument("dedisperse: " + std::to_string(nchans) + " channels of " +
                                        std::to_string(nbits) + "-bit data: rows are not a whole number of bytes");
        return nchans * nbits / 8;
    }
    const size_t esize = dtype == RT_DEDISP_F32 ? 4 : 1;
    if (nchans > SIZE_MAX / esize) throw std::invalid_argument("dedisperse: too many channels");
    return nchans * esize;
}

inline void dedisp_check_flags(uint32_t flags)
{
    if (flags & ~RT_DEDISP_ZERO_DM) throw std::invalid_argument("dedisperse: unknown flag bit");
}

inline void dedisp_check_chan_cap(int dtype, size_t nchans)
{
    if (dedisp_integer_sum(dtype) && nchans > RT_DEDISP_MAX_CHANS_8BIT)
        throw std::invalid_argument("dedisperse: too many channels for an exact 8-bit sum (255 * nchans must be "
                                    "below 2^24)");
}

// a known type (`who` names the caller in that message), at least one channel,
// with `cap` the 8-bit channel cap, packed rows of whole bytes
inline void dedisp_check_dtype(int dtype, size_t nchans, bool cap, const char* who = "dedisperse")
{
    if (!dedisp_known_dtype(dtype)) throw std::invalid_argument(std::string(who) + ": unknown sample type code");
    if (!nchans) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    if (cap) dedisp_check_chan_cap(dtype, nchans);
    if (dedisp_packed_bits(dtype)) dedisp_row_bytes(dtype, nchans);
}

// a band table in host memory: every band a channel range lo <= hi <= nchans
inline void dedisp_check_band_table(const uint32_t* bands, size_t nbands, size_t nchans)
{
    for (size_t b = 0; b < nbands; ++b)
        if (bands[2 * b] > bands[2 * b + 1] || bands[2 * b + 1] > nchans)
            throw std::invalid_argument("dedisperse: band " + std::to_string(b) + " [" +
                                        std::to_string(bands[2 * b]) + ", " + std::to_string(bands[2 * b + 1]) +
                                        ") is not a channel range lo <= hi <= " + std::to_string(nchans));
}

// bytes of one channel's fill of a block mask: the sample's own type, for
// 1/2/4-bit data one unpacked value per byte
constexpr size_t dedisp_fill_bytes(int dtype)
{
    return dtype == RT_DEDISP_F32 ? 4 : dtype == RT_DEDISP_U16 ? 2 : 1;
}

// a block mask (NULL: none) in front of `nsamp` rows from its t_origin: a block
// length, both arrays, and every row inside the nblocks * block_len samples the
// cells cover, so that no load leaves them
inline void dedisp_check_block_mask(const rt_block_mask* bm, size_t nsamp)
{
    if (!bm) return;
    if (!bm->block_len) throw std::invalid_argument("block_mask: block_len must be at least 1");
    if (!bm->cells || !bm->fill) throw std::invalid_argument("block_mask: cells or fill is NULL");
    // t_origin + t is computed in 64 bits everywhere: it must not wrap
    if (bm->t_origin > UINT64_MAX - nsamp)
        throw std::invalid_argument("block_mask: t_origin + nsamp overflows 64 bits");
    const unsigned __int128 covered = (unsigned __int128)bm->nblocks * bm->block_len;
    if ((unsigned __int128)bm->t_origin + nsamp > covered)
        throw std::invalid_argument("block_mask: the rows [" + std::to_string(bm->t_origin) + ", " +
                                    std::to_string(bm->t_origin) + " + " + std::to_string(nsamp) +
                                    ") reach past the mask's " + std::to_string(bm->nblocks) + " blocks of " +
                                    std::to_string(bm->block_len) + " samples");
}

}  // namespace rt
