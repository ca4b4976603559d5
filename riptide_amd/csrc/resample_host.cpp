// C ABI, host-only entry point of the resampling: the specification
// (resample_host.hpp).  No HIP header: this file is also built by g++ with the
// sanitizers (Makefile asan).
#include "riptide_amd.h"

#include "capi_common.hpp"
#include "resample_host.hpp"

using namespace rt;

extern "C" {

int rt_resample_host(const float* x, size_t nseries, size_t size, size_t ldx, const int32_t* src,
                     const double* factor, size_t nrows, float* out, size_t ldo)
{
    return guarded([&] {
        resample_host(x, nseries, size, ldx, src, factor, nrows, out, ldo);
        return RT_OK;
    });
}

}  // extern "C"
