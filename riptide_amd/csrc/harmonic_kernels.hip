// Harmonic flagging for MI355X (gfx950): riptide's htest
// (riptide/pipeline/harmonic_testing.py:90-155) over every pair of a ranked
// cluster list, one lane per pair.
//
//   harmonic_pairs_kernel  rows [i0, i0 + rows) of the pair matrix as bits:
//                          bit j of row i = htest(F = cluster i, H = cluster j)
//                          for j > i, 0 for j <= i; the pairs the host has to
//                          decide (harmonic.hpp hguard) appended to a list
//   harmonic_diag_kernel   hdiag's fraction and three distances of explicit pairs
//
// The arithmetic is harmonic.hpp's, shared with the host.
#include <hip/hip_runtime.h>

#include "harmonic.hpp"
#include "kernels.hpp"

namespace rt {

namespace {

constexpr uint32_t kHBlock = 256;
constexpr uint32_t kHWaves = kHBlock / 64;

__device__ __forceinline__ HCand hload(const double* __restrict__ freq, const double* __restrict__ snr,
                                       const double* __restrict__ ducy, const double* __restrict__ dm, uint32_t i)
{
    HCand c;
    c.freq = freq[i];
    c.snr = snr[i];
    c.ducy = ducy[i];
    c.dm = dm[i];
    return c;
}

}  // namespace

// One wave = one 64-bit word of the tile's row-major bit matrix (wpr words per
// row): lane l of word w of row i tests the pair (i, 64 w + l), the wave's
// ballot is the word, lane 0 stores it.  Words wholly at or left of the
// diagonal are stored as zero without a test.
__global__ __launch_bounds__(kHBlock) void harmonic_pairs_kernel(
    const double* __restrict__ freq, const double* __restrict__ snr, const double* __restrict__ ducy,
    const double* __restrict__ dm, uint32_t n, uint32_t i0, uint32_t rows, uint32_t wpr, HParams P,
    uint64_t* __restrict__ words, uint2* __restrict__ near_list, uint32_t near_cap, uint32_t* __restrict__ near_count)
{
    const uint64_t word = (uint64_t)blockIdx.x * kHWaves + threadIdx.x / 64;   // the same for the whole wave
    if (word >= (uint64_t)rows * wpr) return;
    const uint32_t r = (uint32_t)(word / wpr);
    const uint32_t w = (uint32_t)(word - (uint64_t)r * wpr);
    const uint32_t i = i0 + r;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t j = (uint64_t)w * 64 + lane;
    bool related = false;
    if (j > i && j < n) {
        const HCand F = hload(freq, snr, ducy, dm, i);
        const HCand H = hload(freq, snr, ducy, dm, (uint32_t)j);
        bool near;
        related = htest_pair(F, H, P, &near);
        if (near) {
            const uint32_t at = atomicAdd(near_count, 1u);
            if (at < near_cap) near_list[at] = make_uint2(i, (uint32_t)j);
        }
    }
    const uint64_t mask = __ballot(related);
    if (lane == 0) words[word] = mask;
}

// One thread per pair (pi[k] as F, pj[k] as H).
__global__ __launch_bounds__(kHBlock) void harmonic_diag_kernel(
    const double* __restrict__ freq, const double* __restrict__ snr, const double* __restrict__ ducy,
    const double* __restrict__ dm, const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, uint64_t npairs,
    HParams P, int64_t* __restrict__ num, int64_t* __restrict__ den, double* __restrict__ phase_distance,
    double* __restrict__ dm_distance, double* __restrict__ snr_distance)
{
    const uint64_t k = (uint64_t)blockIdx.x * kHBlock + threadIdx.x;
    if (k >= npairs) return;
    const HDiag d = hdiag_pair(hload(freq, snr, ducy, dm, (uint32_t)pi[k]), hload(freq, snr, ducy, dm, (uint32_t)pj[k]),
                               P);
    num[k] = d.num;
    den[k] = d.den;
    phase_distance[k] = d.phase_distance;
    dm_distance[k] = d.dm_distance;
    snr_distance[k] = d.snr_distance;
}

hipError_t launch_harmonic_pairs(const double* freq, const double* snr, const double* ducy, const double* dm,
                                 uint32_t n, uint32_t i0, uint32_t rows, uint32_t wpr, const HParams& P,
                                 uint64_t* words, uint2* near_list, uint32_t near_cap, uint32_t* near_count,
                                 hipStream_t s)
{
    const uint64_t total = (uint64_t)rows * wpr;
    if (!total) return hipSuccess;
    hipLaunchKernelGGL(harmonic_pairs_kernel, dim3((uint32_t)((total + kHWaves - 1) / kHWaves)), dim3(kHBlock), 0, s,
                       freq, snr, ducy, dm, n, i0, rows, wpr, P, words, near_list, near_cap, near_count);
    return hipGetLastError();
}

hipError_t launch_harmonic_diag(const double* freq, const double* snr, const double* ducy, const double* dm,
                                const int32_t* pi, const int32_t* pj, uint64_t npairs, const HParams& P, int64_t* num,
                                int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance,
                                hipStream_t s)
{
    if (!npairs) return hipSuccess;
    hipLaunchKernelGGL(harmonic_diag_kernel, dim3((uint32_t)((npairs + kHBlock - 1) / kHBlock)), dim3(kHBlock), 0, s,
                       freq, snr, ducy, dm, pi, pj, npairs, P, num, den, phase_distance, dm_distance, snr_distance);
    return hipGetLastError();
}

}  // namespace rt
