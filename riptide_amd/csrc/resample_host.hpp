// Time-domain resampling for the acceleration search: the argument checks, the
// index function and the sequential specification, and the launch shape of the
// device form.  No HIP header: shared by the kernel (resample_kernels.hip), the
// C ABI (capi_resample.cpp, resample_host.cpp) and the sanitizer checker
// (resample_check_main.cpp).
//
// The map.  Output row r is made from source row src[r] of x[B, N] with the
// float64 factor f = factor[r]:
//
//   q_j = j * (N - j)                            exact integer, j = 0 .. N - 1
//   s_j = (int64) rint(f * (double)q_j)          one IEEE double multiply, round-half-even
//   out[r, j] = x[src[r], clamp(j - s_j, 0, N - 1)]
//
// a copy of the float's bits.  N <= 2^27, so q_j <= N^2 / 4 <= 2^52 is exact in
// a double (and equals the double product (double)j * (double)(N - j), which
// the kernel forms: both factors and the product are integers below 2^53).
// |f| * N < 1, so |s_j| < q_j / N <= N / 4, s_{j+1} - s_j is -1, 0 or 1 and the
// source index never decreases; j - s_j lies in [0, N] -- with f just above
// -1 / N, rint carries sample N - 1 to index N -- and is clamped at both ends.
// The shift vanishes towards both ends of the row (q_0 = 0, q_{N-1} = N - 1).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>

#include "capi_common.hpp"

namespace rt {

constexpr uint64_t kResampleMaxSamples = RT_RESAMPLE_MAX_SAMPLES;   // q_j stays exact
constexpr uint64_t kResampleMaxRows = RT_RESAMPLE_MAX_ROWS;         // of one call
constexpr uint32_t kResampleThreads = 256;
constexpr uint32_t kResampleVec = 4;                                // consecutive outputs of one store
constexpr uint32_t kResampleGroups = 2;                             // stores of one lane, a block's width apart
constexpr uint32_t kResampleTile = kResampleThreads * kResampleVec * kResampleGroups;   // outputs of a workgroup
constexpr uint32_t kResampleLaunchRows = RT_RESAMPLE_LAUNCH_ROWS;   // rows of one launch: their table travels as kernel arguments

inline void resample_check_args(const float* x, size_t B, size_t N, size_t ldx, const int32_t* src,
                                const double* factor, size_t R, const float* out, size_t ldo)
{
    if (N > kResampleMaxSamples) throw std::invalid_argument("resample: more than 2^27 samples");
    if (R > kResampleMaxRows) throw std::invalid_argument("resample: more than 65535 rows in a call");
    if (!R || !N) return;
    if (!x || !src || !factor || !out) throw std::invalid_argument("resample: null pointer");
    if (ldx < N) throw std::invalid_argument("resample: input row stride below the series length");
    if (ldo < N) throw std::invalid_argument("resample: output row stride below the series length");
    for (size_t r = 0; r < R; ++r) {
        if (src[r] < 0 || (uint64_t)src[r] >= B) throw std::invalid_argument("resample: source row outside [0, B)");
        if (!std::isfinite(factor[r])) throw std::invalid_argument("resample: a factor is not finite");
        if (std::fabs(factor[r]) * (double)N >= 1.0)
            throw std::invalid_argument("resample: |factor| * N must be below 1");
    }
}

// the source sample of output j
inline uint64_t resample_index(double f, uint64_t j, uint64_t N)
{
    const uint64_t q = j * (N - j);
    const int64_t i = (int64_t)j - (int64_t)std::rint(f * (double)q);
    return i < 0 ? 0 : (uint64_t)i >= N ? N - 1 : (uint64_t)i;
}

// The specification, sequential.  out must not overlap x.
static inline void resample_host(const float* x, size_t B, size_t N, size_t ldx, const int32_t* src,
                                 const double* factor, size_t R, float* out, size_t ldo)
{
    resample_check_args(x, B, N, ldx, src, factor, R, out, ldo);
    if (!N) return;
    for (size_t r = 0; r < R; ++r) {
        const float* row = x + (size_t)src[r] * ldx;
        float* o = out + r * ldo;
        for (size_t j = 0; j < N; ++j) std::memcpy(o + j, row + resample_index(factor[r], j, N), sizeof(float));
    }
}

// ---- the device form: one launch per kResampleLaunchRows rows, grid (tiles, rows)

struct ResampleRows {   // a launch's table, passed by value
    double factor[kResampleLaunchRows];
    int32_t src[kResampleLaunchRows];
};

inline uint32_t resample_tiles(size_t N) { return (uint32_t)((N + kResampleTile - 1) / kResampleTile); }

}  // namespace rt
