// Host-only checker of the candidate refinement (refine_host.hpp through
// rt_refine_shifts and rt_refine_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a read or write past a cube, a table or
// an output is a sanitizer report.  No device call, and none linked.
// Prints "refine_check OK"; exit status 0 iff every call returned what it
// should and the profiles agree with a recomputation in double.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 12345;
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

// shift tables of the physics, then the specification on an integer cube:
// every profile equals the double recomputation exactly
void run_shape(size_t B, size_t S, size_t N, size_t K, size_t J)
{
    std::vector<double> f(B), periods(J), dms(K);
    // unevenly spaced and positive: narrower bands where there are many
    const double df = B > 16 ? 1.25 : 37.0, ddf = B > 16 ? 0.001 : 3.0;
    for (size_t b = 0; b < B; ++b) f[b] = 1500.0 - df * (double)b - ddf * (double)(b * b);
    const double P = 0.5, T = 600.0, dm = 50.0, kdm = 4148.808;
    for (size_t j = 0; j < J; ++j) periods[j] = 1.0 / (1.0 / P - ((double)j - (double)(J / 2)) * 1.7 / ((double)N * T));
    for (size_t k = 0; k < K; ++k) dms[k] = dm + ((double)k - (double)(K / 2)) * 900.0;
    std::vector<int32_t> ps(J * S), ds(K * B);
    expect(rt_refine_shifts(P, T, N, S, f.data(), B, dm, kdm, periods.data(), J, dms.data(), K, ps.data(),
                            ds.data()) == RT_OK, "rt_refine_shifts");
    for (int32_t v : ps) expect(v >= 0 && (size_t)v < N, "pshift in range");
    for (int32_t v : ds) expect(v >= 0 && (size_t)v < N, "dshift in range");
    // 0 and N - 1 side by side: the double wrap
    ps[0] = (int32_t)(N - 1);
    ds[0] = (int32_t)(N - 1);
    if (S > 1) ps[1] = 0;
    if (B > 1) ds[1] = 0;
    std::vector<uint32_t> widths{1u, (uint32_t)(N - 1), (uint32_t)((N + 1) / 2)};
    if (N == 2) widths = {1u};
    const size_t W = widths.size();
    std::vector<float> x(B * S * N), snr(K * J * W), prof(K * J * N);
    for (float& v : x) v = (float)((int)(uniform() * 17.0) - 8);
    expect(rt_refine_host(x.data(), B, S, N, ds.data(), K, ps.data(), J, widths.data(), W, 1.5f, snr.data(),
                          prof.data()) == RT_OK, "rt_refine_host");
    for (size_t k = 0; k < K; ++k)
        for (size_t j = 0; j < J; ++j)
            for (size_t n = 0; n < N; ++n) {
                double acc = 0.0;
                for (size_t b = 0; b < B; ++b)
                    for (size_t s = 0; s < S; ++s)
                        acc += (double)x[(b * S + s) * N + (n + (size_t)ds[k * B + b] + (size_t)ps[j * S + s]) % N];
                if ((double)prof[(k * J + j) * N + n] != acc) {
                    std::printf("FAILED: profile (%zu, %zu, %zu) of shape %zu x %zu x %zu\n", k, j, n, B, S, N);
                    g_failed = 1;
                    return;
                }
            }
    for (float v : snr) expect(std::isfinite(v), "finite S/N");
    // without the profile output
    std::vector<float> snr2(K * J * W);
    expect(rt_refine_host(x.data(), B, S, N, ds.data(), K, ps.data(), J, widths.data(), W, 1.5f, snr2.data(),
                          nullptr) == RT_OK, "rt_refine_host without profiles");
    expect(!std::memcmp(snr.data(), snr2.data(), snr.size() * sizeof(float)), "S/N with and without profiles");
}

void run_errors()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    std::vector<double> f{1400.0, 1300.0}, per{0.5, 0.5001}, dms{10.0, 11.0};
    std::vector<int32_t> ps(2 * 3), ds(2 * 2);
    auto shifts = [&](double P, double T, size_t N, size_t S, size_t B, size_t J, size_t K) {
        return rt_refine_shifts(P, T, N, S, f.data(), B, 10.0, 4148.808, per.data(), J, dms.data(), K, ps.data(),
                                ds.data());
    };
    expect(shifts(0.5, 100.0, 16, 3, 2, 2, 2) == RT_OK, "shifts baseline");
    for (double bad : {0.0, -1.0, inf, nan}) {
        expect(shifts(bad, 100.0, 16, 3, 2, 2, 2) == RT_EINVAL, "bad period");
        expect(shifts(0.5, bad, 16, 3, 2, 2, 2) == RT_EINVAL, "bad span");
        const double keep = per[1];
        per[1] = bad;
        expect(shifts(0.5, 100.0, 16, 3, 2, 2, 2) == RT_EINVAL, "bad trial period");
        per[1] = keep;
        const double keepf = f[0];
        f[0] = bad;
        expect(shifts(0.5, 100.0, 16, 3, 2, 2, 2) == RT_EINVAL, "bad frequency");
        f[0] = keepf;
    }
    expect(shifts(0.5, 100.0, 1, 3, 2, 2, 2) == RT_EINVAL, "bins 1");
    expect(shifts(0.5, 100.0, 16, 0, 2, 2, 2) == RT_EINVAL, "subints 0");
    expect(shifts(0.5, 100.0, 16, 3, 0, 2, 2) == RT_EINVAL, "bands 0");
    expect(shifts(0.5, 100.0, 16, 3, 2, 0, 2) == RT_EINVAL, "periods 0");
    expect(shifts(0.5, 100.0, 16, 3, 2, 2, 0) == RT_EINVAL, "dms 0");
    dms[1] = 1e30;
    expect(shifts(0.5, 100.0, 16, 3, 2, 2, 2) == RT_EINVAL, "DM shift of 2^31 or more");
    dms[1] = nan;
    expect(shifts(0.5, 100.0, 16, 3, 2, 2, 2) == RT_EINVAL, "DM that is not finite");
    dms[1] = 11.0;
    per[1] = 1e-12;
    expect(shifts(0.5, 1e6, 16, 3, 2, 2, 2) == RT_EINVAL, "period shift of 2^31 or more");
    per[1] = 0.5001;

    const size_t B = 2, S = 3, N = 5, K = 2, J = 2;
    std::vector<float> x(B * S * N, 1.0f), snr(K * J * 2);
    std::vector<int32_t> d(K * B, 0), p(J * S, 0);
    std::vector<uint32_t> w{1u, 4u};
    auto host = [&](float stdnoise) {
        return rt_refine_host(x.data(), B, S, N, d.data(), K, p.data(), J, w.data(), w.size(), stdnoise, snr.data(),
                              nullptr);
    };
    expect(host(1.0f) == RT_OK, "host baseline");
    d[3] = (int32_t)N;
    expect(host(1.0f) == RT_EINVAL, "DM shift of N");
    d[3] = -1;
    expect(host(1.0f) == RT_EINVAL, "negative DM shift");
    d[3] = 0;
    p[5] = (int32_t)N;
    expect(host(1.0f) == RT_EINVAL, "period shift of N");
    p[5] = 0;
    w[1] = 0;
    expect(host(1.0f) == RT_EINVAL, "width 0");
    w[1] = (uint32_t)N;
    expect(host(1.0f) == RT_EINVAL, "width N");
    w[1] = 4;
    expect(host(0.0f) == RT_EINVAL, "stdnoise 0");
    expect(host(-1.0f) == RT_EINVAL, "stdnoise below 0");
    expect(rt_refine_host(x.data(), B, S, 1, d.data(), K, p.data(), J, w.data(), 2, 1.0f, snr.data(), nullptr) ==
               RT_EINVAL, "host bins 1");
    expect(rt_refine_host(x.data(), B, S, N, d.data(), K, p.data(), J, w.data(), 0, 1.0f, snr.data(), nullptr) ==
               RT_EINVAL, "host no widths");
    expect(rt_refine_host(x.data(), B, S, N, d.data(), 0, p.data(), J, w.data(), 2, 1.0f, snr.data(), nullptr) ==
               RT_EINVAL, "host no DM trials");

    rt_refine_spec sp{};
    sp.bands = 2; sp.subints = 3; sp.bins = 5; sp.ndm = 2; sp.nper = 2; sp.nw = 2; sp.stdnoise = 1.0f;
    size_t bytes = 0;
    expect(rt_refine_workspace_bytes(&sp, 1, &bytes) == RT_OK && bytes >= 2 * 3 * 5 * 4, "workspace bytes");
    sp.bins = 1025;
    expect(rt_refine_workspace_bytes(&sp, 1, &bytes) == RT_EINVAL, "workspace: bins above 1024");
    sp.bins = 5;
    sp.stdnoise = 0.0f;
    expect(rt_refine_workspace_bytes(&sp, 1, &bytes) == RT_EINVAL, "workspace: stdnoise 0");
}

}  // namespace

int main()
{
    run_shape(1, 1, 2, 1, 1);
    run_shape(2, 1, 3, 3, 2);
    run_shape(7, 2, 65, 3, 3);
    run_shape(3, 33, 64, 3, 3);
    run_shape(7, 2, 257, 5, 3);
    // more than 256 rows of each table, and 700 bins (tests/test_refine_host.py)
    run_shape(513, 2, 31, 3, 3);
    run_shape(2, 513, 16, 3, 3);
    run_shape(3, 2, 700, 2, 2);
    run_errors();
    if (g_failed) return 1;
    std::printf("refine_check OK\n");
    return 0;
}
