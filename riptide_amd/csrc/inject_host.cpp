// C ABI, host-only entry points of the signal injection: the checks and the
// specification (inject_host.hpp).  No HIP header: this file is also built by
// g++ with the sanitizers (Makefile asan).
#include "riptide_amd.h"

#include "capi_common.hpp"
#include "inject_host.hpp"

using namespace rt;

extern "C" {

int rt_inject_check(int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, const rt_inject_spec* specs,
                    size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp, size_t amp_len,
                    const int32_t* delay, size_t delay_len)
{
    return guarded([&] {
        inject_check(dtype, nsamp, nchans, t_origin, specs, nspecs, tmpl, tmpl_len, amp, amp_len, delay, delay_len);
        return RT_OK;
    });
}

int rt_inject_host(void* x, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
                   const rt_inject_spec* specs, size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp,
                   size_t amp_len, const int32_t* delay, size_t delay_len)
{
    return guarded([&] {
        inject_host(x, dtype, nsamp, nchans, t_origin, seed, specs, nspecs, tmpl, tmpl_len, amp, amp_len, delay,
                    delay_len);
        return RT_OK;
    });
}

}  // extern "C"
