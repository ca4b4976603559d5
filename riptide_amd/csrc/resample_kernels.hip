// Time-domain resampling for MI355X (gfx950): the map of resample_host.hpp
// for a batch of (source row, factor) rows, device-resident.
//
//   resample_kernel   grid (tile of outputs, output row).  A lane makes
//                     kResampleGroups groups of kResampleVec = 4 consecutive
//                     outputs, a workgroup's width apart, and stores each group
//                     with one 16-byte store when the output row starts on a
//                     16-byte boundary (four 4-byte stores otherwise).
//
// A gather: every output is the bits of one input, so host and device agree
// bit for bit as long as the index does.  The index: q_j as the double product
// (double)j * (double)(N - j) -- exact, both factors and the product are
// integers below 2^53 -- then the one rounded multiply f * q_j, rint
// (v_rndne_f64, round-half-even) and a clamp.  The build's -ffp-contract=off
// is not even needed: there is no addition to contract with.
//
// The reads are near unit stride: consecutive outputs read consecutive inputs
// except where s_j steps by one, so a wave's 4-byte loads fall into the cache
// lines of one contiguous span and each input line is fetched once.  The row's
// factor and source are wave-uniform: they come out of the kernel arguments
// through scalar loads indexed by blockIdx.y.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rt {

namespace {

// resample_index of resample_host.hpp in 32-bit indices (N <= 2^27, |s_j| < N / 4)
__device__ __forceinline__ uint32_t resample_src(double f, uint32_t j, uint32_t N)
{
    const double q = (double)j * (double)(N - j);
    const int32_t i = (int32_t)j - (int32_t)rint(f * q);
    return (uint32_t)min(max(i, 0), (int32_t)N - 1);
}

__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const float* __restrict__ x, uint64_t ldx,
                                                                    uint32_t N, ResampleRows T,
                                                                    float* __restrict__ out, uint64_t ldo)
{
    const uint32_t r = blockIdx.y;
    const double f = T.factor[r];
    // the samples as their bits: nothing here is arithmetic on them
    const uint32_t* row = reinterpret_cast<const uint32_t*>(x) + (uint64_t)T.src[r] * ldx;
    uint32_t* o = reinterpret_cast<uint32_t*>(out) + (uint64_t)r * ldo;
    const bool aligned = ((uintptr_t)o & 15) == 0;
    const uint32_t base = blockIdx.x * kResampleTile + threadIdx.x * kResampleVec;

    uint32_t v[kResampleGroups][kResampleVec];
#pragma unroll
    for (uint32_t g = 0; g < kResampleGroups; ++g) {
        const uint32_t j0 = base + g * kResampleThreads * kResampleVec;
#pragma unroll
        for (uint32_t k = 0; k < kResampleVec; ++k)
            // every lane loads (past the row's end: sample N - 1 again, never stored), so the
            // loads of a lane go out together
            v[g][k] = row[resample_src(f, min(j0 + k, N - 1), N)];
    }
#pragma unroll
    for (uint32_t g = 0; g < kResampleGroups; ++g) {
        const uint32_t j0 = base + g * kResampleThreads * kResampleVec;
        if (aligned && j0 + kResampleVec <= N) {
            *reinterpret_cast<uint4*>(o + j0) = make_uint4(v[g][0], v[g][1], v[g][2], v[g][3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kResampleVec; ++k)
                if (j0 + k < N) o[j0 + k] = v[g][k];
        }
    }
}

}  // namespace

hipError_t launch_resample(const float* x, uint64_t ldx, uint32_t N, const ResampleRows& T, uint32_t rows,
                           float* out, uint64_t ldo, hipStream_t s)
{
    if (!rows || !N) return hipSuccess;
    hipLaunchKernelGGL(resample_kernel, dim3(resample_tiles(N), rows), dim3(kResampleThreads), 0, s, x, ldx, N, T,
                       out, ldo);
    return hipGetLastError();
}

}  // namespace rt
