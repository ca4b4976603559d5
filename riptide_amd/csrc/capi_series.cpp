// C ABI, time-series side: the host-buffer drop-ins for riptide.libcpp's
// array functions (rollback, prefix sum, S/N, downsampling, running medians)
// and dereddening + normalisation, host-buffer and device-resident.
#include "riptide_amd.h"

#include <mutex>
#include <stdexcept>
#include <vector>

#include "capi_device.hpp"
#include "dered_host.hpp"
#include "kernels.hpp"
#include "plan.hpp"

using namespace rt;

namespace {

void run_deredden_normalise(const float* d_in, size_t size, size_t batch, size_t in_stride, const DeredGeom& g,
                            bool deredden, bool normalise, float* d_out, size_t out_stride, void* ws, hipStream_t s)
{
    const DeredWs w = dered_ws_layout(ws, g);
    const float* cur = d_in;
    size_t cur_stride = in_stride;
    const bool fused = deredden && normalise && g.sf > 1 &&
                       dered_norm_fusable(d_in, size, g.n_lo, (uint32_t)g.sf, d_out, in_stride, out_stride);
    if (deredden) {
        const float* rin = d_in;
        size_t rstride = in_stride;
        if (g.sf > 1) {
            ck(launch_scrunch(d_in, g.n_lo, (uint32_t)g.sf, w.lores, in_stride, g.n_lo, (uint32_t)batch, s), "scrunch");
            rin = w.lores;
            rstride = g.n_lo;
        }
        ck(launch_running_median(rin, g.n_lo, (uint32_t)g.rmed_w, w.rmed, rstride, g.n_lo, (uint32_t)batch, s),
           "running_median");
        if (fused) {
            const size_t np = 2 * dered_norm_blocks(size) * batch;
            ck(launch_deredden_normalise(d_in, size, w.rmed, g.n_lo, (uint32_t)g.sf, d_out, in_stride, g.n_lo,
                                         out_stride, (uint32_t)batch, s, w.slopes, w.partials, w.partials + np),
               "deredden_normalise");
            return;
        }
        ck(launch_deredden_subtract(d_in, size, w.rmed, g.n_lo, (uint32_t)g.sf, d_out, in_stride, g.n_lo, out_stride,
                                    (uint32_t)batch, s, g.slope_doubles ? w.slopes : nullptr),
           "deredden_subtract");
        cur = d_out;
        cur_stride = out_stride;
    }
    if (normalise) {
        ck(launch_normalise(cur, size, d_out, w.partials, kNormBlocks, cur_stride, out_stride, (uint32_t)batch, s),
           "normalise");
    } else if (!deredden && cur != d_out) {
        for (size_t b = 0; b < batch; ++b)
            ck(hipMemcpyAsync(d_out + b * out_stride, d_in + b * in_stride, size * 4, hipMemcpyDeviceToDevice, s),
               "copy");
    }
}

}  // namespace

extern "C" {

int rt_rollback(const float* x, size_t size, size_t shift, float* out)
{
    return guarded([&] {
        if (!size) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_rollback(dx, size, shift, nullptr, dz, c.stream), "rollback");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_fused_rollback_add(const float* x, const float* y, size_t size, size_t shift, float* out)
{
    return guarded([&] {
        if (!size) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dy = dev<float>(c, 1, size);
        float* dz = dev<float>(c, 2, size);
        h2d(dx, x, size * 4, c.stream);
        h2d(dy, y, size * 4, c.stream);
        ck(launch_rollback(dx, size, shift, dy, dz, c.stream), "fused_rollback_add");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_circular_prefix_sum(const float* x, size_t size, size_t nsum, float* out)
{
    return guarded([&] {
        if (!nsum) return RT_OK;
        if (!size) throw std::invalid_argument("circular_prefix_sum of an empty array");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, nsum + 1);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_circular_prefix_sum(dx, size, nsum, dz, c.stream), "circular_prefix_sum");
        d2h(out, dz, nsum * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_snr2(const float* x, size_t rows, size_t cols, const uint64_t* widths, size_t nw, float stdnoise, float* out)
{
    return guarded([&] {
        if (!(stdnoise > 0)) throw std::invalid_argument("stdnoise must be > 0");
        check_widths(widths, nw, cols);
        if (!rows || !nw) return RT_OK;
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        const size_t n = rows * cols;
        float* dx = dev<float>(c, 0, n);
        float* dc = dev<float>(c, 1, n + rows);
        uint32_t* dw = dev<uint32_t>(c, 2, nw);
        float* dz = dev<float>(c, 3, rows * nw);
        std::vector<uint32_t> w32(widths, widths + nw);
        h2d(dx, x, n * 4, c.stream);
        h2d(dw, w32.data(), nw * 4, c.stream);
        ck(launch_snr_rows(dx, rows, (uint32_t)cols, dw, (uint32_t)nw, stdnoise, dc, dz, c.stream), "snr");
        d2h(out, dz, rows * nw * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_snr1(const float* x, size_t size, const uint64_t* widths, size_t nw, float stdnoise, float* out)
{
    return rt_snr2(x, 1, size, widths, nw, stdnoise, out);
}

size_t rt_downsampled_size(size_t size, double f) { return downsampled_size(size, f); }

int rt_downsample_rows(const float* x, size_t rows, size_t size, double f, float* out)
{
    return guarded([&] {
        // downsample.hpp:11-16
        if (!((f > 1.0) & (f <= (double)size)))
            throw std::invalid_argument("Downsampling factor must verify: 1 < f <= size");
        if (!rows) return RT_OK;
        if (rows > 65535) throw std::invalid_argument("at most 65535 rows per call");
        const size_t n = downsampled_size(size, f);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, rows * size);
        float* dz = dev<float>(c, 1, rows * n);
        DsRung* dr = dev<DsRung>(c, 2, 1);
        DsRung r{};
        r.f = f;
        r.n = n;
        r.first_block = 0;
        ds_configure(r);
        h2d(dx, x, rows * size * 4, c.stream);
        h2d(dr, &r, sizeof r, c.stream);
        ck(launch_downsample_ladder(dx, size, size, dr, 1, (uint32_t)((n + r.per_block - 1) / r.per_block), dz, n,
                                    (uint32_t)rows, c.stream),
           "downsample");
        d2h(out, dz, rows * n * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

// one row: the factor check comes first there too
int rt_downsample(const float* x, size_t size, double f, float* out) { return rt_downsample_rows(x, 1, size, f, out); }

int rt_running_median(const float* x, size_t size, size_t width, float* out)
{
    return guarded([&] {
        // running_median.hpp:103-107
        if (!(width % 2)) throw std::invalid_argument("width must be an odd number");
        if (!(width < size)) throw std::invalid_argument("width must be < size");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_running_median(dx, size, (uint32_t)width, dz, size, size, 1, c.stream), "running_median");
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_fast_running_median(const float* x, size_t size, size_t ws, size_t minpts, double* out)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, 1, true);
        if (g.sf == 1) throw std::invalid_argument("scrunch factor is 1: use rt_running_median");
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        double* dz = dev<double>(c, 1, size);
        float* lores = dev<float>(c, 2, g.n_lo);
        float* rmed = dev<float>(c, 3, g.n_lo);
        h2d(dx, x, size * 4, c.stream);
        ck(launch_scrunch(dx, g.n_lo, (uint32_t)g.sf, lores, size, g.n_lo, 1, c.stream), "scrunch");
        ck(launch_running_median(lores, g.n_lo, (uint32_t)g.rmed_w, rmed, g.n_lo, g.n_lo, 1, c.stream),
           "running_median");
        ck(launch_interp(size, rmed, g.n_lo, (uint32_t)g.sf, dz, c.stream), "interp");
        d2h(out, dz, size * 8, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_deredden_normalise(const float* x, size_t size, size_t ws, size_t minpts, int deredden, int normalise,
                          float* out)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, 1, deredden != 0);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        float* dx = dev<float>(c, 0, size);
        float* dz = dev<float>(c, 1, size);
        void* w = c.buf[2].get(dered_ws_bytes(g));
        h2d(dx, x, size * 4, c.stream);
        run_deredden_normalise(dx, size, 1, size, g, deredden != 0, normalise != 0, dz, size, w, c.stream);
        d2h(out, dz, size * 4, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

int rt_deredden_normalise_device(const float* d_in, size_t size, size_t batch, size_t in_stride, size_t ws,
                                 size_t minpts, int deredden, int normalise, float* d_out, size_t out_stride,
                                 void* d_ws, size_t ws_bytes, void* stream)
{
    return guarded([&] {
        const DeredGeom g = dered_geom(size, ws, minpts, batch, deredden != 0);
        if (ws_bytes < dered_ws_bytes(g)) throw std::invalid_argument("workspace too small");
        if (deredden && d_in == d_out) throw std::invalid_argument("deredden cannot run in place");
        run_deredden_normalise(d_in, size, batch, in_stride, g, deredden != 0, normalise != 0, d_out, out_stride,
                               d_ws, (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_convert_samples_device(const void* d_raw, size_t n, int is_signed, float* d_out, void* stream)
{
    return guarded([&] {
        if (n >= (1ull << 42)) throw std::invalid_argument("too many samples");
        ck(launch_convert_samples(d_raw, n, is_signed, d_out, (hipStream_t)stream), "convert_samples");
        return RT_OK;
    });
}

}  // extern "C"
