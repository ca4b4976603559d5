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

// whether the transposed rows of the workspace are float32 (float and 16-bit
// data, and every type under the zero-DM filter) or 8-bit
constexpr bool dedisp_float_rows(int dtype, uint32_t flags)
{
    return (flags & RT_DEDISP_ZERO_DM) || !dedisp_integer_sum(dtype);
}

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

// ---- the staging rule of dedisp_sum_kernel (dedisp_kernels.hip), which takes
// these numbers and dedisp_span from here; rt_dedisperse_span_plan
// (dedisp_host.cpp) is the same function, for tests to name the path they run.
// A workgroup sums kDedispTile outputs from t0, a multiple of kDedispTile, of
// 16 DMs.  Per channel, with lo and hi the smallest and largest clamped delay
// of those DMs, it reads the elements [t0 + lo, t0 + kDedispTile + hi) of the
// channel's row.  That span, from the dword holding its first element, is
// staged in LDS when it fits the dwords below, and read from the workspace row
// directly otherwise:
//   8-bit rows  staged iff hi - (lo & ~3) <= 800: a spread hi - lo of up to
//               800, 799, 798, 797 samples for lo % 4 = 0, 1, 2, 3
//   float rows  staged iff hi - lo <= 264
constexpr uint32_t kDedispTile = 256;            // outputs of a time tile
constexpr uint32_t kDedispSpanDwords8 = 264;     // staged dwords of a channel, 8-bit rows
constexpr uint32_t kDedispSpanDwords32 = 520;    // the same, float rows

constexpr uint32_t dedisp_span_dwords(uint32_t esize) { return esize == 1 ? kDedispSpanDwords8 : kDedispSpanDwords32; }

struct DedispSpan {
    uint32_t first;   // first element staged: the span's first element rounded down to a dword
    uint32_t ndw;     // dwords from there to the span's end
    bool direct;      // ndw is more than the LDS span holds: the channel is read from its row
};

// esize: bytes of a row's element, 1 or 4.  e_lo = t0 + lo and e_hi = t0 + hi
// in the kernel; t0 is a multiple of 256, so the plan of (lo, hi) alone has
// the same ndw and path (first is then relative to t0).  e_hi + 256 must not
// overflow 32 bits: blocks and delays are below 2^31.
constexpr DedispSpan dedisp_span(uint32_t esize, uint32_t e_lo, uint32_t e_hi)
{
    const uint32_t per = 4 / esize;                  // elements per dword
    const uint32_t e0 = e_lo & ~(per - 1);           // first element staged
    const uint32_t e1 = e_hi + kDedispTile;          // one past the last element read
    const uint32_t ndw = (e1 - e0 + per - 1) / per;
    return DedispSpan{e0, ndw, ndw > dedisp_span_dwords(esize)};
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

// the shape limits of a resident-block call: the kernels' 32-bit indices and grids
inline void dedisp_check_shape(int dtype, size_t nsamp_blk, size_t nchans, size_t ndm, int64_t max_delay)
{
    if (!dedisp_known_dtype(dtype)) throw std::invalid_argument("dedisperse: unknown sample type code");
    if (!nchans || !ndm) throw std::invalid_argument("dedisperse: nchans and ndm must be at least 1");
    dedisp_check_chan_cap(dtype, nchans);
    if (nchans > 65535ull * 64) throw std::invalid_argument("dedisperse: too many channels");
    if (ndm > 65535ull * 16) throw std::invalid_argument("dedisperse: too many DMs for one call");
    if (nsamp_blk >= (1ull << 31)) throw std::invalid_argument("dedisperse: a block must be below 2^31 samples");
    // packed rows: whole bytes, and nsamp_blk * row_bytes inside the kernels' 64-bit byte offsets
    // (row_bytes < 2^23 by the channel limit above)
    if (dedisp_packed_bits(dtype) && dedisp_row_bytes(dtype, nchans) > (~0ull >> 1) / (nsamp_blk ? nsamp_blk : 1))
        throw std::invalid_argument("dedisperse: the block's bytes overflow a 64-bit offset");
    if (max_delay < 0 || (uint64_t)max_delay >= nsamp_blk)
        throw std::invalid_argument("dedisperse: max_delay must be in [0, nsamp): the block is no longer than the "
                                    "largest delay");
}

// ---- decimated steps (riptide_amd.h: rt_dedisperse_ds_host, rt_dedisp_step)
inline void dedisp_check_downsamp(uint64_t f)
{
    if (f < 1 || f > RT_DEDISP_MAX_DOWNSAMP)
        throw std::invalid_argument("dedisperse: downsamp " + std::to_string(f) + " is outside [1, " +
                                    std::to_string(RT_DEDISP_MAX_DOWNSAMP) + "]");
}

// the exactness cap of a step of factor f: integer sums stay below 2^24
inline void dedisp_check_ds_cap(int dtype, size_t nchans, uint64_t f, uint32_t flags)
{
    if (!dedisp_integer_sum(dtype) || (flags & RT_DEDISP_ZERO_DM)) return;
    const int nbits = dedisp_packed_bits(dtype);
    const uint64_t vmax = nbits ? (1ull << nbits) - 1 : 255;
    if (vmax * f * nchans >= (1ull << 24))   // f <= 256, nchans < 2^23: no overflow
        throw std::invalid_argument("dedisperse: " + std::to_string(nchans) + " channels at downsamp " +
                                    std::to_string(f) + " are too many for an exact sum (" + std::to_string(vmax) +
                                    " * downsamp * nchans must be below 2^24)");
}

// a block mask in front of decimated steps: every gulp starts on a decimated sample
inline void dedisp_check_mask_origin(const rt_block_mask* bm, uint64_t f)
{
    if (bm && bm->t_origin % f)
        throw std::invalid_argument("block_mask: t_origin " + std::to_string(bm->t_origin) +
                                    " is not a multiple of downsamp " + std::to_string(f));
}

// a step table in host memory over a block of nsamp_blk rows (rt_dedisperse_steps_check)
inline void dedisp_check_steps(int dtype, size_t nsamp_blk, size_t nchans, const rt_dedisp_step* steps,
                               size_t nsteps, size_t delays_len, size_t out_floats, uint32_t flags,
                               const rt_block_mask* bm)
{
    dedisp_check_flags(flags);
    dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
    dedisp_check_block_mask(bm, nsamp_blk);
    if (!steps || !nsteps) throw std::invalid_argument("dedisperse: a step table needs at least one step");
    for (size_t k = 0; k < nsteps; ++k) {
        const rt_dedisp_step& st = steps[k];
        const std::string who = "dedisperse: step " + std::to_string(k) + ": ";
        dedisp_check_downsamp(st.downsamp);
        if (st.reserved) throw std::invalid_argument(who + "reserved must be 0");
        if (!st.ndm) throw std::invalid_argument(who + "ndm must be at least 1");
        if (st.ndm > 65535ull * 16) throw std::invalid_argument("dedisperse: too many DMs for one call");
        const uint64_t nz = nsamp_blk / st.downsamp;
        if (st.max_delay >= nz)
            throw std::invalid_argument(who + "max_delay " + std::to_string(st.max_delay) + " is not below the " +
                                        std::to_string(nz) + " decimated samples of the block");
        dedisp_check_mask_origin(bm, st.downsamp);
        dedisp_check_ds_cap(dtype, nchans, st.downsamp, flags);
        const uint64_t nout = nz - st.max_delay;
        if (st.delays_off > delays_len || (uint64_t)st.ndm * nchans > delays_len - st.delays_off)
            throw std::invalid_argument(who + "its delay table leaves the delay array");
        if (st.out_offset > st.out_stride || nout > st.out_stride - st.out_offset)
            throw std::invalid_argument(who + "out_stride is shorter than out_offset plus the step's outputs");
        // the last float written: out_off + (ndm - 1) * out_stride + out_offset + nout - 1
        const unsigned __int128 end = (unsigned __int128)st.out_off +
                                      (unsigned __int128)(st.ndm - 1) * st.out_stride + st.out_offset + nout;
        if (end > out_floats) throw std::invalid_argument(who + "its output rows leave the output array");
    }
}

}  // namespace rt
