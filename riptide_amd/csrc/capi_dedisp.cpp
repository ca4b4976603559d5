// C ABI, filterbank side: incoherent dedispersion, the zero-DM filter and the
// channel statistics, with the shape limits of their kernels' 32-bit indices
// and grids.  The seven dedispersion calls are two cores, the resident-block
// one and the host-buffer one, each with an optional band table; the
// resident-block core also takes an optional block mask (rt_block_mask), as
// the zero-DM mean does, and the block statistics stand beside the channel
// statistics.  The step-table calls (rt_dedisperse_steps*: the steps of a DM
// plan, each decimated in time) check their table with dedisp_check_steps of
// dedisp_types.hpp, which the host-only rt_dedisperse_steps_check shares.
#include "riptide_amd.h"

#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "capi_dedisp.hpp"
#include "capi_device.hpp"
#include "dedisp_types.hpp"
#include "kernels.hpp"

using namespace rt;

namespace {

// (the shape limits of a call, dedisp_check_shape, and the step table's checks: dedisp_types.hpp)

// The band table of the band forms, in device memory for the resident-block
// call and in host memory for the host-buffer one; no BandTable (a null
// pointer to one) is the plain form.
struct BandTable {
    const uint32_t* table;
    size_t nbands;
};

// the band forms: every band a grid layer, every (DM, band) a row of out
void dedisp_check_bands(size_t ndm, size_t nbands)
{
    if (!nbands) throw std::invalid_argument("dedisperse: nbands must be at least 1");
    if (nbands > RT_DEDISP_MAX_BANDS)
        throw std::invalid_argument("dedisperse: too many bands for one call (at most " +
                                    std::to_string(RT_DEDISP_MAX_BANDS) + ")");
    if (ndm * nbands > 0xFFFFFFFFull)   // ndm < 2^20, nbands < 2^16: no overflow here
        throw std::invalid_argument("dedisperse: ndm * nbands rows overflow 32 bits");
}

// rt_dedisperse_device, _device_opt, rt_dedisperse_bands_device (bt->table in
// device memory) and rt_dedisperse_device_cells (bm: cells and fill in device
// memory)
int dedisperse_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const int32_t* d_delays,
                      const uint8_t* d_mask, size_t ndm, const BandTable* bt, int64_t max_delay, float* d_out,
                      size_t out_stride, size_t out_offset, void* d_ws, size_t ws_bytes, void* stream, uint32_t flags,
                      const rt_block_mask* bm = nullptr)
{
    return guarded([&] {
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp_blk, nchans, ndm, max_delay);
        const DeviceCells dc(bm, dtype, nsamp_blk);
        if (bt) dedisp_check_bands(ndm, bt->nbands);
        const size_t nout = nsamp_blk - (size_t)max_delay;
        if (out_offset > out_stride || nout > out_stride - out_offset)
            throw std::invalid_argument("dedisperse: out_stride is shorter than out_offset plus the block's outputs");
        if (!d_block || !d_delays || !d_out || !d_ws) throw std::invalid_argument("dedisperse: null device pointer");
        if (bt && !bt->table) throw std::invalid_argument("dedisperse: d_bands is NULL");
        if ((uintptr_t)d_ws % 16 || (bt && (uintptr_t)bt->table % 4) ||
            (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("dedisperse: misaligned device pointer");
        if (ws_bytes < dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags))
            throw std::invalid_argument("workspace too small");
        ck(launch_dedisperse(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_delays, d_mask, (uint32_t)ndm,
                             (uint32_t)max_delay, d_out + out_offset, out_stride, d_ws, flags, (hipStream_t)stream,
                             bt ? bt->table : nullptr, bt ? (uint32_t)bt->nbands : 0u, dc.get()),
           "dedisperse");
        return RT_OK;
    });
}

// rt_dedisperse, _opt and rt_dedisperse_bands (bt->table in host memory): the
// delays narrowed to int32, everything uploaded into the context's buffers
// (slot 5: the band table), the kernels, the rows copied out
int dedisperse_buffers(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                       const uint8_t* mask, size_t ndm, const BandTable* bt, int64_t max_delay, float* out,
                       uint32_t flags)
{
    return guarded([&] {
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp, nchans, ndm, max_delay);
        if (bt) dedisp_check_bands(ndm, bt->nbands);
        if (!x || !delays || !out || (bt && !bt->table)) throw std::invalid_argument("dedisperse: null buffer");
        if (bt) dedisp_check_band_table(bt->table, bt->nbands, nchans);
        std::vector<int32_t> del(ndm * nchans);
        for (size_t i = 0; i < del.size(); ++i) {
            if (delays[i] < 0 || delays[i] > max_delay)
                throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
            del[i] = (int32_t)delays[i];
        }
        const size_t nout = nsamp - (size_t)max_delay;
        const size_t nrows = ndm * (bt ? bt->nbands : 1);
        const size_t in_bytes = nsamp * dedisp_row_bytes(dtype, nchans);
        const size_t ws_bytes = (size_t)dedisp_workspace_bytes(dtype, nsamp, nchans, flags);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        void* dx = c.buf[0].get(in_bytes);
        float* dz = dev<float>(c, 1, nrows * nout);
        void* dw = c.buf[2].get(ws_bytes);
        int32_t* dd = dev<int32_t>(c, 3, del.size());
        uint8_t* dm = mask ? dev<uint8_t>(c, 4, nchans) : nullptr;
        uint32_t* db = bt ? dev<uint32_t>(c, 5, 2 * bt->nbands) : nullptr;
        h2d(dx, x, in_bytes, c.stream);
        h2d(dd, del.data(), del.size() * 4, c.stream);
        if (mask) h2d(dm, mask, nchans, c.stream);
        if (bt) h2d(db, bt->table, 2 * bt->nbands * 4, c.stream);
        ck(launch_dedisperse(dx, dtype, (uint32_t)nsamp, (uint32_t)nchans, dd, dm, (uint32_t)ndm,
                             (uint32_t)max_delay, dz, nout, dw, flags, c.stream, db, bt ? (uint32_t)bt->nbands : 0u),
           "dedisperse");
        d2h(out, dz, nrows * nout * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

// the smallest downsamp > 1 of a list of factors (0: none): what sizes the decimated area
uint32_t steps_min_factor(const uint32_t* factors, size_t n)
{
    uint32_t fmin = 0;
    for (size_t i = 0; i < n; ++i) {
        dedisp_check_downsamp(factors[i]);
        if (factors[i] > 1 && (!fmin || factors[i] < fmin)) fmin = factors[i];
    }
    return fmin;
}

uint64_t steps_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, const rt_dedisp_step* steps,
                               size_t nsteps, uint32_t flags)
{
    std::vector<uint32_t> factors(nsteps);
    for (size_t k = 0; k < nsteps; ++k) factors[k] = steps[k].downsamp;
    return dedisp_steps_workspace_bytes(dtype, nsamp_blk, nchans, flags, steps_min_factor(factors.data(), nsteps));
}

// the statistics have no exactness limit on the channel count of 8-bit data
void chanstats_check_shape(int dtype, size_t nsamp_blk, size_t nchans)
{
    dedisp_check_shape(RT_DEDISP_F32, nsamp_blk, nchans, 1, 0);
    if (!dedisp_known_dtype(dtype)) throw std::invalid_argument("channel_stats: unknown sample type code");
    if (dedisp_packed_bits(dtype)) dedisp_row_bytes(dtype, nchans);
}

// The block length the statistics kernels run with: a block longer than the
// resident block is the same single block, so the length stays below 2^31
// and the grid's x (at most nsamp_blk workgroups, or a few per 2048 rows)
// below 2^31 too.
size_t blockstats_block_len(size_t nsamp_blk, size_t block_len)
{
    if (!block_len) throw std::invalid_argument("block_stats: block_len must be at least 1");
    return block_len < nsamp_blk ? block_len : nsamp_blk;
}

}  // namespace

extern "C" {

int rt_dedisperse_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, size_t* bytes)
{
    return rt_dedisperse_workspace_bytes_opt(dtype, nsamp_blk, nchans, 0u, bytes);
}

int rt_dedisperse_workspace_bytes_opt(int dtype, size_t nsamp_blk, size_t nchans, uint32_t flags, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("dedisperse: bytes is NULL");
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
        *bytes = (size_t)dedisp_workspace_bytes(dtype, nsamp_blk, nchans, flags);
        return RT_OK;
    });
}

int rt_dedisperse_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const int32_t* d_delays,
                         const uint8_t* d_mask, size_t ndm, int64_t max_delay, float* d_out, size_t out_stride,
                         size_t out_offset, void* d_ws, size_t ws_bytes, void* stream)
{
    return dedisperse_device(d_block, dtype, nsamp_blk, nchans, d_delays, d_mask, ndm, nullptr, max_delay, d_out,
                             out_stride, out_offset, d_ws, ws_bytes, stream, 0u);
}

int rt_dedisperse_device_opt(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                             const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, int64_t max_delay,
                             float* d_out, size_t out_stride, size_t out_offset, void* d_ws, size_t ws_bytes,
                             void* stream, uint32_t flags)
{
    return dedisperse_device(d_block, dtype, nsamp_blk, nchans, d_delays, d_mask, ndm, nullptr, max_delay, d_out,
                             out_stride, out_offset, d_ws, ws_bytes, stream, flags);
}

int rt_dedisperse_bands_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, const uint32_t* d_bands,
                               size_t nbands, int64_t max_delay, float* d_out, size_t out_stride, size_t out_offset,
                               void* d_ws, size_t ws_bytes, void* stream, uint32_t flags)
{
    const BandTable bt{d_bands, nbands};
    return dedisperse_device(d_block, dtype, nsamp_blk, nchans, d_delays, d_mask, ndm, &bt, max_delay, d_out,
                             out_stride, out_offset, d_ws, ws_bytes, stream, flags);
}

int rt_dedisperse(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays, const uint8_t* mask,
                  size_t ndm, int64_t max_delay, float* out)
{
    return dedisperse_buffers(x, dtype, nsamp, nchans, delays, mask, ndm, nullptr, max_delay, out, 0u);
}

int rt_dedisperse_opt(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                      const uint8_t* mask, size_t ndm, int64_t max_delay, float* out, uint32_t flags)
{
    return dedisperse_buffers(x, dtype, nsamp, nchans, delays, mask, ndm, nullptr, max_delay, out, flags);
}

int rt_dedisperse_bands(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                        const uint8_t* mask, size_t ndm, const uint32_t* bands, size_t nbands, int64_t max_delay,
                        float* out, uint32_t flags)
{
    const BandTable bt{bands, nbands};
    return dedisperse_buffers(x, dtype, nsamp, nchans, delays, mask, ndm, &bt, max_delay, out, flags);
}

int rt_dedisperse_device_cells(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, const uint32_t* d_bands,
                               size_t nbands, int64_t max_delay, float* d_out, size_t out_stride, size_t out_offset,
                               void* d_ws, size_t ws_bytes, void* stream, uint32_t flags, const rt_block_mask* bm)
{
    const BandTable bt{d_bands, nbands};
    return dedisperse_device(d_block, dtype, nsamp_blk, nchans, d_delays, d_mask, ndm,
                             d_bands || nbands ? &bt : nullptr, max_delay, d_out, out_stride, out_offset, d_ws,
                             ws_bytes, stream, flags, bm);
}

int rt_dedisperse_steps_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, const uint32_t* factors,
                                        size_t nfactors, uint32_t flags, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("dedisperse: bytes is NULL");
        if (nfactors && !factors) throw std::invalid_argument("dedisperse: factors is NULL");
        dedisp_check_flags(flags);
        dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
        *bytes = (size_t)dedisp_steps_workspace_bytes(dtype, nsamp_blk, nchans, flags,
                                                      steps_min_factor(factors, nfactors));
        return RT_OK;
    });
}

int rt_dedisperse_steps_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, size_t delays_len, const uint8_t* d_mask,
                               const rt_dedisp_step* steps, size_t nsteps, float* d_out, size_t out_floats,
                               void* d_ws, size_t ws_bytes, void* stream, uint32_t flags, const rt_block_mask* bm)
{
    return guarded([&] {
        dedisp_check_steps(dtype, nsamp_blk, nchans, steps, nsteps, delays_len, out_floats, flags, bm);
        const DeviceCells dc(bm, dtype, nsamp_blk);
        if (!d_block || !d_delays || !d_out || !d_ws) throw std::invalid_argument("dedisperse: null device pointer");
        if ((uintptr_t)d_ws % 16 || (uintptr_t)d_delays % 4 || (uintptr_t)d_out % 4 ||
            (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("dedisperse: misaligned device pointer");
        if (ws_bytes < steps_workspace_bytes(dtype, nsamp_blk, nchans, steps, nsteps, flags))
            throw std::invalid_argument("workspace too small");
        ck(launch_dedisperse_steps(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_delays, d_mask, steps,
                                   nsteps, d_out, d_ws, flags, (hipStream_t)stream, dc.get()),
           "dedisperse");
        return RT_OK;
    });
}

int rt_dedisperse_steps(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                        size_t delays_len, const uint8_t* mask, const rt_dedisp_step* steps, size_t nsteps,
                        float* out, size_t out_floats, uint32_t flags)
{
    return guarded([&] {
        dedisp_check_steps(dtype, nsamp, nchans, steps, nsteps, delays_len, out_floats, flags, nullptr);
        if (!x || !delays || !out) throw std::invalid_argument("dedisperse: null buffer");
        std::vector<int32_t> del(delays_len);
        for (size_t k = 0; k < nsteps; ++k) {   // tables that overlap are checked once per step
            const rt_dedisp_step& st = steps[k];
            for (size_t i = st.delays_off; i < st.delays_off + (size_t)st.ndm * nchans; ++i) {
                if (delays[i] < 0 || delays[i] > (int64_t)st.max_delay)
                    throw std::invalid_argument("dedisperse: a delay is outside [0, max_delay]");
                del[i] = (int32_t)delays[i];
            }
        }
        const size_t in_bytes = nsamp * dedisp_row_bytes(dtype, nchans);
        const size_t ws_bytes = (size_t)steps_workspace_bytes(dtype, nsamp, nchans, steps, nsteps, flags);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        void* dx = c.buf[0].get(in_bytes);
        float* dz = dev<float>(c, 1, out_floats);
        void* dw = c.buf[2].get(ws_bytes);
        int32_t* dd = dev<int32_t>(c, 3, del.size());
        uint8_t* dm = mask ? dev<uint8_t>(c, 4, nchans) : nullptr;
        h2d(dx, x, in_bytes, c.stream);
        h2d(dz, out, out_floats * 4, c.stream);   // what no step writes comes back as it was
        h2d(dd, del.data(), del.size() * 4, c.stream);
        if (mask) h2d(dm, mask, nchans, c.stream);
        ck(launch_dedisperse_steps(dx, dtype, (uint32_t)nsamp, (uint32_t)nchans, dd, dm, steps, nsteps, dz, dw, flags,
                                   c.stream),
           "dedisperse");
        d2h(out, dz, out_floats * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_zero_dm_mean_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const uint8_t* d_mask,
                           float* d_m, void* stream)
{
    return rt_zero_dm_mean_device_cells(d_block, dtype, nsamp_blk, nchans, d_mask, d_m, stream, nullptr);
}

int rt_zero_dm_mean_device_cells(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                                 const uint8_t* d_mask, float* d_m, void* stream, const rt_block_mask* bm)
{
    return guarded([&] {
        dedisp_check_shape(dtype, nsamp_blk, nchans, 1, 0);
        const DeviceCells dc(bm, dtype, nsamp_blk);
        if (!d_block || !d_m) throw std::invalid_argument("zero_dm_mean: null device pointer");
        if ((uintptr_t)d_m % 4 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("zero_dm_mean: misaligned device pointer");
        ck(launch_zero_dm_mean(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_mask, d_m,
                               (hipStream_t)stream, dc.get()),
           "zero_dm_mean");
        return RT_OK;
    });
}

int rt_block_stats_workspace_bytes(size_t nsamp_blk, size_t nchans, size_t block_len, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("block_stats: bytes is NULL");
        chanstats_check_shape(RT_DEDISP_F32, nsamp_blk, nchans);
        *bytes = (size_t)blockstats_workspace_bytes(nsamp_blk, nchans, blockstats_block_len(nsamp_blk, block_len));
        return RT_OK;
    });
}

int rt_block_stats_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, size_t block_len,
                          double* d_stats, void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        chanstats_check_shape(dtype, nsamp_blk, nchans);
        const size_t blen = blockstats_block_len(nsamp_blk, block_len);
        const uint64_t need = blockstats_workspace_bytes(nsamp_blk, nchans, blen);
        if (!d_block || !d_stats || (need && !d_ws)) throw std::invalid_argument("block_stats: null device pointer");
        if ((uintptr_t)d_stats % 8 || (uintptr_t)d_ws % 8 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("block_stats: misaligned device pointer");
        if (ws_bytes < need) throw std::invalid_argument("workspace too small");
        ck(launch_block_stats(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, (uint32_t)blen, d_stats, d_ws,
                              (hipStream_t)stream),
           "block_stats");
        return RT_OK;
    });
}

int rt_channel_stats_workspace_bytes(size_t nsamp_blk, size_t nchans, size_t* bytes)
{
    return guarded([&] {
        if (!bytes) throw std::invalid_argument("channel_stats: bytes is NULL");
        chanstats_check_shape(RT_DEDISP_F32, nsamp_blk, nchans);
        *bytes = (size_t)chanstats_workspace_bytes(nsamp_blk, nchans);
        return RT_OK;
    });
}

int rt_channel_stats_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, double* d_acc,
                            void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        chanstats_check_shape(dtype, nsamp_blk, nchans);
        if (!d_block || !d_acc || !d_ws) throw std::invalid_argument("channel_stats: null device pointer");
        if ((uintptr_t)d_acc % 8 || (uintptr_t)d_ws % 8 || (dtype == RT_DEDISP_F32 && (uintptr_t)d_block % 4))
            throw std::invalid_argument("channel_stats: misaligned device pointer");
        if (ws_bytes < chanstats_workspace_bytes(nsamp_blk, nchans))
            throw std::invalid_argument("workspace too small");
        ck(launch_channel_stats(d_block, dtype, (uint32_t)nsamp_blk, (uint32_t)nchans, d_acc, d_ws,
                                (hipStream_t)stream),
           "channel_stats");
        return RT_OK;
    });
}

}  // extern "C"
