// Host-only checker of the single-pulse specification (pulse_host.hpp through
// rt_single_pulse_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a read or write past a row, the event
// list or a dense output is a sanitizer report.  No device call, and none
// linked.  Prints "pulse_check OK"; exit status 0 iff every call returned what
// it should and the results agree with a direct recomputation on integer data.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 2024;
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

// integer samples: every sum is exact, so best / kbest / events must equal
// the plain loops below
void run_shape(size_t B, size_t N, size_t ldx, std::vector<int32_t> w, size_t R, float thr, size_t cap)
{
    // rows of exactly ldx floats except the last, which has N
    std::vector<float> x((B - 1) * ldx + N);
    for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < (b + 1 < B ? ldx : N); ++i)
            x[b * ldx + i] = i < N ? (float)((int)(uniform() * 9.0) - 4) : std::nanf("");
    const size_t K = w.size();
    std::vector<float> best(B * N);
    std::vector<int32_t> kbest(B * N);
    std::vector<rt_pulse_event> ev(cap);
    uint64_t count = ~0ull;
    expect(rt_single_pulse_host(x.data(), B, N, ldx, w.data(), K, thr, R, cap ? ev.data() : nullptr, cap, &count,
                                best.data(), kbest.data()) == RT_OK, "rt_single_pulse_host");
    uint64_t found = 0;
    for (size_t b = 0; b < B; ++b) {
        std::vector<float> bv(N);
        for (size_t t = 0; t < N; ++t) {
            float m = -std::numeric_limits<float>::infinity();
            int32_t mk = -1;
            for (size_t k = 0; k < K; ++k) {
                const size_t wk = (size_t)w[k], c = wk / 2;
                if (t < c || t - c + wk > N) continue;
                double acc = 0.0;
                for (size_t i = t - c; i < t - c + wk; ++i) acc += (double)x[b * ldx + i];
                const float s = (float)(acc / std::sqrt((double)wk));
                if (s > m) {
                    m = s;
                    mk = (int32_t)k;
                }
            }
            bv[t] = m;
            if (best[b * N + t] != m || kbest[b * N + t] != mk) {
                std::printf("FAILED: best (%zu, %zu) of %zu x %zu\n", b, t, B, N);
                g_failed = 1;
                return;
            }
        }
        for (size_t t = 0; t < N; ++t) {
            bool is = bv[t] >= thr;
            for (size_t u = t > R ? t - R : 0; is && u < t; ++u) is = bv[t] > bv[u];
            for (size_t u = t + 1; is && u < N && u <= t + R; ++u) is = bv[t] >= bv[u];
            if (!is) continue;
            if (found < cap) {
                const rt_pulse_event& e = ev[found];
                expect(e.series == (int32_t)b && e.sample == (int32_t)t && e.iwidth == kbest[b * N + t] &&
                           e.snr == bv[t], "event record");
            }
            ++found;
        }
    }
    expect(count == found, "event count");
    // events only, and dense only
    uint64_t count2 = 0;
    expect(rt_single_pulse_host(x.data(), B, N, ldx, w.data(), K, thr, R, cap ? ev.data() : nullptr, cap, &count2,
                                nullptr, nullptr) == RT_OK && count2 == found, "events without dense outputs");
    expect(rt_single_pulse_host(x.data(), B, N, ldx, w.data(), K, thr, R, nullptr, 0, nullptr, best.data(),
                                nullptr) == RT_OK, "dense output alone");
}

void run_errors()
{
    std::vector<float> x(64, 0.5f);
    std::vector<rt_pulse_event> ev(4);
    uint64_t count = 0;
    auto call = [&](std::vector<int32_t> w, size_t N, float thr, size_t R, size_t ldx) {
        return rt_single_pulse_host(x.data(), 1, N, ldx, w.data(), w.size(), thr, R, ev.data(), ev.size(), &count,
                                    nullptr, nullptr);
    };
    expect(call({1, 2, 4}, 64, 3.0f, 4, 64) == RT_OK, "baseline");
    expect(call({}, 64, 3.0f, 4, 64) == RT_EINVAL, "no widths");
    expect(call({0, 2}, 64, 3.0f, 4, 64) == RT_EINVAL, "width 0");
    expect(call({-3, 2}, 64, 3.0f, 4, 64) == RT_EINVAL, "width below 0");
    expect(call({2, 2}, 64, 3.0f, 4, 64) == RT_EINVAL, "equal widths");
    expect(call({4, 2}, 64, 3.0f, 4, 64) == RT_EINVAL, "descending widths");
    expect(call({1, 65}, 64, 3.0f, 4, 64) == RT_EINVAL, "width above N");
    expect(call({1, RT_PULSE_MAX_WIDTH + 1}, 64, 3.0f, 4, 64) == RT_EINVAL, "width above the limit");
    expect(call({1, 2}, 64, 3.0f, RT_PULSE_MAX_WIDTH + 1, 64) == RT_EINVAL, "radius above the limit");
    expect(call({1, 2}, 64, std::numeric_limits<float>::infinity(), 4, 64) == RT_EINVAL, "infinite threshold");
    expect(call({1, 2}, 64, std::nanf(""), 4, 64) == RT_EINVAL, "NaN threshold");
    expect(call({1, 2}, 64, 3.0f, 4, 63) == RT_EINVAL, "stride below N");
    expect(rt_single_pulse_host(x.data(), 1, 64, 64, nullptr, 2, 3.0f, 4, ev.data(), 4, &count, nullptr, nullptr) ==
               RT_EINVAL, "null widths");
    const int32_t w[2] = {1, 2};
    expect(rt_single_pulse_host(x.data(), 1, 64, 64, w, 2, 0.0f, 4, nullptr, 4, &count, nullptr, nullptr) ==
               RT_EINVAL, "null events with a capacity");
    size_t tile = 0, mw = 0, bytes = 0;
    expect(rt_single_pulse_limits(&tile, &mw) == RT_OK && tile >= 1024 && mw == RT_PULSE_MAX_WIDTH, "limits");
    expect(rt_single_pulse_workspace_bytes(3, 10000, 5, 100, &bytes) == RT_OK && bytes >= 100 * sizeof(rt_pulse_event),
           "workspace bytes");
    expect(rt_single_pulse_workspace_bytes(3, 10000, 0, 100, &bytes) == RT_EINVAL, "workspace: no widths");
    size_t chunk = 0, segs = 0, lds = 0;
    expect(rt_single_pulse_plan(RT_PULSE_MAX_WIDTH, RT_PULSE_MAX_WIDTH, &chunk, &segs, &lds) == RT_OK && chunk >= 1024 &&
               chunk % RT_PULSE_SEGMENT == 0 && segs == (chunk + RT_PULSE_MAX_WIDTH + 2045) / 1024 &&
               lds <= (160u << 10) && lds > segs * 8 * 1088, "plan at the limits");
    expect(rt_single_pulse_plan(1, 0, nullptr, nullptr, nullptr) == RT_OK, "plan: null outputs");
    expect(rt_single_pulse_plan(0, 4, &chunk, &segs, &lds) == RT_EINVAL, "plan: width 0");
    expect(rt_single_pulse_plan(RT_PULSE_MAX_WIDTH + 1, 4, &chunk, &segs, &lds) == RT_EINVAL,
           "plan: width above the limit");
    expect(rt_single_pulse_plan(64, RT_PULSE_MAX_WIDTH + 1, &chunk, &segs, &lds) == RT_EINVAL,
           "plan: radius above the limit");
}

}  // namespace

int main()
{
    run_shape(1, 64, 64, {1, 2, 3, 4, 6, 9, 13, 19, 28, 42, 64}, 8, 2.0f, 64);      // N equal to the largest width
    run_shape(1, 50, 50, {1, 2, 5}, 200, 1.0f, 50);                                 // R larger than N
    run_shape(1, 1, 1, {1}, 0, -100.0f, 1);                                         // one sample
    run_shape(3, 1500, 1511, {1, 2, 3, 4, 6, 9, 33, 700}, 5, 3.0f, 4096);           // ldx > N, crosses a segment
    run_shape(2, 2300, 2300, {1, 16, 17, 1024, 1025, 2200}, 30, 4.0f, 7);           // whole segments inside a window
    run_shape(2, 300, 307, {1, 2, 4}, 3, 0.5f, 0);                                  // a capacity of zero
    run_errors();
    if (g_failed) return 1;
    std::printf("pulse_check OK\n");
    return 0;
}
