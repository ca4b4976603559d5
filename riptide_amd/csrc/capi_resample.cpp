// C ABI, resampling of device series: the checks of resample_host.hpp, then
// one launch per RT_RESAMPLE_LAUNCH_ROWS rows with the rows' table as kernel
// arguments -- no staging buffer, no workspace.
#include "riptide_amd.h"

#include <algorithm>

#include "capi_device.hpp"
#include "kernels.hpp"
#include "resample_host.hpp"

using namespace rt;

extern "C" {

int rt_resample_device(const float* d_x, size_t nseries, size_t size, size_t ldx, const int32_t* src,
                       const double* factor, size_t nrows, float* d_out, size_t ldo, void* stream)
{
    return guarded([&] {
        resample_check_args(d_x, nseries, size, ldx, src, factor, nrows, d_out, ldo);
        if (!nrows || !size) return RT_OK;
        hipStream_t s = (hipStream_t)stream;
        for (size_t r0 = 0; r0 < nrows; r0 += kResampleLaunchRows) {
            const uint32_t rows = (uint32_t)std::min<size_t>(kResampleLaunchRows, nrows - r0);
            ResampleRows T{};
            std::copy(src + r0, src + r0 + rows, T.src);
            std::copy(factor + r0, factor + r0 + rows, T.factor);
            ck(launch_resample(d_x, ldx, (uint32_t)size, T, rows, d_out + r0 * ldo, ldo, s), "resample");
        }
        return RT_OK;
    });
}

}  // extern "C"
