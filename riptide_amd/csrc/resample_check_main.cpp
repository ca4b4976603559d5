// Host-only checker of the resampling specification (resample_host.hpp through
// rt_resample_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a read past a source row (the clamp) or a
// write past an output row is a sanitizer report.  No device call, and none
// linked.  Prints "resample_check OK"; exit status 0 iff every call returned
// what it should and the rows agree with a direct recomputation.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 2025;
double uniform()   // 53-bit LCG draw in [0, 1)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int g_failed = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, rt_last_error());
        g_failed = 1;
    }
}

// the unclamped source index of output j
int64_t wanted(double f, int64_t j, int64_t N) { return j - (int64_t)std::nearbyint(f * (double)(j * (N - j))); }

// R rows of B sources: rows of exactly ldx / ldo floats except the last, which has N
void run_shape(size_t B, size_t N, size_t ldx, size_t ldo, const std::vector<double>& factors)
{
    const size_t R = factors.size();
    std::vector<float> x((B - 1) * ldx + N);
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < (b + 1 < B ? ldx : N); ++i)
            x[b * ldx + i] = i < N ? (float)(b * 1000003 + i) : std::nanf("");
    std::vector<int32_t> src(R);
    for (size_t r = 0; r < R; ++r) src[r] = (int32_t)((r * 7 + 3) % B);
    const float canary = -12345.0f;
    std::vector<float> out((R - 1) * ldo + N, canary);
    expect(rt_resample_host(x.data(), B, N, ldx, src.data(), factors.data(), R, out.data(), ldo) == RT_OK,
           "rt_resample_host");
    for (size_t r = 0; r < R; ++r) {
        for (size_t j = 0; j < (r + 1 < R ? ldo : N); ++j) {
            float want = canary;
            if (j < N) {
                int64_t i = wanted(factors[r], (int64_t)j, (int64_t)N);
                i = i < 0 ? 0 : i >= (int64_t)N ? (int64_t)N - 1 : i;
                want = x[(size_t)src[r] * ldx + (size_t)i];
            }
            if (std::memcmp(&want, &out[r * ldo + j], 4)) {
                std::printf("FAILED: (%zu, %zu) of %zu x %zu, factor %.17g\n", r, j, R, N, factors[r]);
                g_failed = 1;
                return;
            }
        }
    }
}

void run_sizes()
{
    for (size_t N : {1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 4099, 65537}) {
        const double edge = (1.0 - std::ldexp(1.0, -20)) / (double)N;
        std::vector<double> f = {0.0, 1e-300, -1e-300, edge, -edge, (2.0 * uniform() - 1.0) * edge};
        if (N == 1025) {
            f.push_back(std::ldexp(1.0, -11));
            f.push_back(-std::ldexp(1.0, -11));
        }
        run_shape(1, N, N, N, f);
        run_shape(5, N, N + 3, N + 5, f);
        // the negative edge factor asks sample N - 1 for index N: the clamp is what keeps the read inside
        // (from N = 3: |f| * q_{N-1} is just under (N - 1) / N, which must exceed 1/2 to round to 1)
        if (N > 2) expect(wanted(-edge, (int64_t)N - 1, (int64_t)N) == (int64_t)N, "the edge factor reaches index N");
    }
    // f * q = 0.5 exactly at j = 1 of N = 1025: half-even gives shift 0
    expect(std::ldexp(1.0, -11) * 1024.0 == 0.5 && wanted(std::ldexp(1.0, -11), 1, 1025) == 1, "the tie rounds to even");
}

void run_errors()
{
    std::vector<float> x(2 * 64, 0.5f), out(3 * 64);
    const int32_t src[3] = {0, 1, 1};
    const double f[3] = {0.0, 1e-3, -1e-3};
    auto call = [&](size_t B, size_t N, size_t ldx, const int32_t* s, const double* ff, size_t R, size_t ldo) {
        return rt_resample_host(x.data(), B, N, ldx, s, ff, R, out.data(), ldo);
    };
    expect(call(2, 64, 64, src, f, 3, 64) == RT_OK, "baseline");
    expect(call(2, 64, 63, src, f, 3, 64) == RT_EINVAL, "input stride below N");
    expect(call(2, 64, 64, src, f, 3, 63) == RT_EINVAL, "output stride below N");
    expect(call(1, 64, 64, src, f, 3, 64) == RT_EINVAL, "source row at B");
    const int32_t neg[3] = {0, -1, 1};
    expect(call(2, 64, 64, neg, f, 3, 64) == RT_EINVAL, "source row below 0");
    for (double bad : {std::nan(""), std::numeric_limits<double>::infinity(), 1.0 / 64.0, -1.0 / 64.0, 1.0}) {
        const double g[3] = {0.0, bad, 0.0};
        expect(call(2, 64, 64, src, g, 3, 64) == RT_EINVAL, "factor refused");
    }
    const double just[3] = {std::nextafter(1.0 / 64.0, 0.0), -std::nextafter(1.0 / 64.0, 0.0), 0.0};
    expect(call(2, 64, 64, src, just, 3, 64) == RT_OK, "the largest factor passes");
    expect(call(2, 64, 64, nullptr, f, 3, 64) == RT_EINVAL, "null src");
    expect(call(2, 64, 64, src, nullptr, 3, 64) == RT_EINVAL, "null factors");
    expect(rt_resample_host(nullptr, 2, 64, 64, src, f, 3, out.data(), 64) == RT_EINVAL, "null input");
    expect(rt_resample_host(x.data(), 2, 64, 64, src, f, 3, nullptr, 64) == RT_EINVAL, "null output");
    // nothing to do: no pointer is looked at
    expect(rt_resample_host(nullptr, 0, 64, 0, nullptr, nullptr, 0, nullptr, 0) == RT_OK, "no rows");
    expect(rt_resample_host(nullptr, 2, 0, 0, nullptr, nullptr, 3, nullptr, 0) == RT_OK, "no samples");
    expect(rt_resample_host(x.data(), 1, (size_t)RT_RESAMPLE_MAX_SAMPLES + 1, (size_t)RT_RESAMPLE_MAX_SAMPLES + 1, src,
                            f, 1, out.data(), (size_t)RT_RESAMPLE_MAX_SAMPLES + 1) == RT_EINVAL, "more than 2^27 samples");
    expect(rt_resample_host(x.data(), 2, 64, 64, src, f, (size_t)RT_RESAMPLE_MAX_ROWS + 1, out.data(), 64) == RT_EINVAL,
           "too many rows");
}

}  // namespace

int main()
{
    run_sizes();
    run_errors();
    if (g_failed) return 1;
    std::printf("resample_check OK\n");
    return 0;
}
