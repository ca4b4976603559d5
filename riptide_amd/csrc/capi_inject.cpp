// C ABI, signal injection into a device block: the table checks of
// inject_host.hpp, then one launch -- no staging buffer, no workspace.  The
// tables are device memory the caller uploaded; the host-buffer form uploads
// them itself.
#include "riptide_amd.h"

#include <stdexcept>

#include "capi_device.hpp"
#include "inject_host.hpp"
#include "kernels.hpp"

using namespace rt;

namespace {

void run_inject(void* d_block, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
                size_t nspecs, const rt_inject_spec* d_specs, const float* d_tmpl, const float* d_amp,
                const int32_t* d_delay, hipStream_t s)
{
    if (!nspecs || !nsamp || !nchans) return;
    if (!d_block || !d_specs || !d_tmpl || !d_amp || !d_delay) throw std::invalid_argument("inject: null device pointer");
    if (((uintptr_t)d_specs & 7) || ((uintptr_t)d_tmpl & 3) || ((uintptr_t)d_amp & 3) || ((uintptr_t)d_delay & 3))
        throw std::invalid_argument("inject: a misaligned table");
    if (dtype == RT_DEDISP_F32 && ((uintptr_t)d_block & 3))
        throw std::invalid_argument("inject: a float32 block must be 4-byte aligned");
    const InjectShape S = inject_shape(dtype, nsamp, nchans, (uintptr_t)d_block);
    if (S.blocks > 0x7fffffffull) throw std::invalid_argument("inject: the block is too large for one launch");
    InjectArgs A{};
    A.x = (char*)d_block - S.m;
    A.specs = d_specs;
    A.tmpl = d_tmpl;
    A.amp = d_amp;
    A.delay = d_delay;
    A.salt = seed * kInjectGolden;
    A.t_origin = (int64_t)t_origin;
    A.nspecs = (uint32_t)nspecs;
    A.nchans = (uint32_t)nchans;
    A.nsamp = (uint32_t)nsamp;
    A.m = S.m;
    A.super_rows = S.super_rows;
    A.col_blocks = S.col_blocks;
    ck(launch_inject(dtype, A, (uint32_t)S.blocks, s), "inject");
}

}  // namespace

extern "C" {

int rt_inject_device(void* d_block, int dtype, size_t nsamp_blk, size_t nchans, uint64_t t_origin, uint64_t seed,
                     const rt_inject_spec* specs, size_t nspecs, const rt_inject_spec* d_specs, const float* d_tmpl,
                     size_t tmpl_len, const float* d_amp, size_t amp_len, const int32_t* d_delay, size_t delay_len,
                     void* stream)
{
    return guarded([&] {
        inject_check_table(dtype, nsamp_blk, nchans, t_origin, specs, nspecs, tmpl_len, amp_len, delay_len);
        if (nspecs > 0xffffffffull) throw std::invalid_argument("inject: too many signals");
        run_inject(d_block, dtype, nsamp_blk, nchans, t_origin, seed, nspecs, d_specs, d_tmpl, d_amp, d_delay,
                   (hipStream_t)stream);
        return RT_OK;
    });
}

int rt_inject(void* x, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
              const rt_inject_spec* specs, size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp,
              size_t amp_len, const int32_t* delay, size_t delay_len)
{
    return guarded([&] {
        inject_check(dtype, nsamp, nchans, t_origin, specs, nspecs, tmpl, tmpl_len, amp, amp_len, delay, delay_len);
        if (!nspecs || !nsamp || !nchans) return RT_OK;
        if (!x) throw std::invalid_argument("inject: null block");
        if (nspecs > 0xffffffffull) throw std::invalid_argument("inject: too many signals");
        const size_t bytes = nsamp * nchans * (dtype == RT_DEDISP_F32 ? 4 : 1);
        std::lock_guard<std::mutex> lk(g_mu);
        Context& c = context();
        void* dx = c.buf[0].get(bytes);
        rt_inject_spec* ds = dev<rt_inject_spec>(c, 1, nspecs);
        float* dt = dev<float>(c, 2, tmpl_len);
        float* da = dev<float>(c, 3, amp_len);
        int32_t* dd = dev<int32_t>(c, 4, delay_len);
        h2d(dx, x, bytes, c.stream);
        h2d(ds, specs, nspecs * sizeof(rt_inject_spec), c.stream);
        h2d(dt, tmpl, tmpl_len * 4, c.stream);
        h2d(da, amp, amp_len * 4, c.stream);
        h2d(dd, delay, delay_len * 4, c.stream);
        run_inject(dx, dtype, nsamp, nchans, t_origin, seed, nspecs, ds, dt, da, dd, c.stream);
        d2h(x, dx, bytes, c.stream);
        sync(c.stream);
        return RT_OK;
    });
}

}  // extern "C"
