// Host-only checker of the signal injection (inject_host.hpp through
// rt_inject_check and rt_inject_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a template gather, an amplitude or a
// delay read past its range, or a write past the block is a sanitizer report,
// and so is any integer step that is not the wrapping arithmetic the
// specification names.  No device call, and none linked.  Prints
// "inject_check OK"; exit status 0 iff every call returned what it should,
// a block cut in two overlapping pieces gives the whole block's bytes, and a
// refused call wrote nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 2026;
uint64_t draw()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return g_state >> 11;
}
double uniform() { return (double)draw() / 9007199254740992.0; }

int g_failed = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, rt_last_error());
        g_failed = 1;
    }
}

struct Tables {
    std::vector<rt_inject_spec> specs;
    std::vector<float> tmpl, amp;
    std::vector<int32_t> delay;
};

// K signals of both kinds over nchans channels; g rows from t_origin are what the pulse windows straddle
Tables make_tables(size_t K, size_t nchans, size_t g, uint64_t t_origin, uint32_t log2bins, double factor,
                   uint64_t span)
{
    Tables T;
    for (size_t k = 0; k < K; ++k) {
        rt_inject_spec sp{};
        sp.kind = (uint32_t)(k & 1);
        const size_t entries = sp.kind == 0 ? (size_t)1 << log2bins : 1 + (size_t)(draw() % 40);
        sp.log2bins = sp.kind == 0 ? log2bins : 0;
        sp.length = sp.kind == 1 ? (uint32_t)entries : 0;
        sp.tmpl_off = T.tmpl.size();
        for (size_t i = 0; i < entries; ++i) T.tmpl.push_back((float)(uniform() * 2.0 - 0.5));
        sp.amp_off = T.amp.size();
        for (size_t c = 0; c < nchans; ++c) T.amp.push_back((float)((uniform() - 0.5) * 8.0));
        sp.delay_off = T.delay.size();
        // delays from far below to far above the block's length
        for (size_t c = 0; c < nchans; ++c) T.delay.push_back((int32_t)(draw() % (4 * g + 7)) - (int32_t)g);
        sp.step = draw() << 11 | 1;
        sp.phase0 = ~0ull - (draw() & 0xffff);   // wraps within a few samples
        // windows before row 0, across it, inside, across the end and past it
        sp.t0 = (int64_t)t_origin + (int64_t)(draw() % (g + 60)) - 30;
        sp.factor = (k % 3 == 2) ? -factor : (k % 3 == 1) ? factor : 0.0;
        sp.span = span;
        T.specs.push_back(sp);
    }
    return T;
}

int call_host(void* x, int dtype, size_t g, size_t nchans, uint64_t t_origin, uint64_t seed, const Tables& T)
{
    return rt_inject_host(x, dtype, g, nchans, t_origin, seed, T.specs.data(), T.specs.size(), T.tmpl.data(),
                          T.tmpl.size(), T.amp.data(), T.amp.size(), T.delay.data(), T.delay.size());
}

void run_shape(int dtype, size_t nchans, size_t g, uint64_t t_origin, size_t K, uint32_t log2bins, double factor,
               uint64_t span)
{
    const size_t es = dtype == RT_DEDISP_F32 ? 4 : 1;
    const Tables T = make_tables(K, nchans, g, t_origin, log2bins, factor, span);
    std::vector<uint8_t> x(g * nchans * es);
    for (size_t i = 0; i < g * nchans; ++i) {
        if (es == 4) {
            const float v = (float)(uniform() * 10.0);
            std::memcpy(&x[4 * i], &v, 4);
        } else {
            x[i] = (uint8_t)(draw() % 7 < 2 ? (draw() & 1 ? 255 : 0) : draw());
        }
    }
    std::vector<uint8_t> whole(x);
    expect(call_host(whole.data(), dtype, g, nchans, t_origin, 7, T) == RT_OK, "rt_inject_host");
    if (!K) expect(whole == x, "no signal leaves the block unchanged");
    // the same block as two overlapping pieces with their t_origin
    const size_t cut = g / 2, over = g > 4 ? 2 : 0;
    std::vector<uint8_t> a(x.begin(), x.begin() + (cut + over) * nchans * es);
    std::vector<uint8_t> b(x.begin() + cut * nchans * es, x.end());
    expect(call_host(a.data(), dtype, cut + over, nchans, t_origin, 7, T) == RT_OK, "first piece");
    expect(call_host(b.data(), dtype, g - cut, nchans, t_origin + cut, 7, T) == RT_OK, "second piece");
    if (!std::equal(a.begin(), a.end(), whole.begin()) || !std::equal(b.begin(), b.end(), whole.begin() + cut * nchans * es)) {
        std::printf("FAILED: pieces differ from the whole (dtype %d, %zu x %zu, K %zu)\n", dtype, g, nchans, K);
        g_failed = 1;
    }
}

void run_shapes()
{
    for (int dtype : {RT_DEDISP_U8, RT_DEDISP_I8, RT_DEDISP_F32})
        for (size_t nchans : {1, 3, 63, 64, 65, 130})
            for (size_t g : {1, 63, 257})
                for (uint64_t t_origin : {0ull, 1000ull}) {
                    const uint64_t span = 4096;
                    const double edge = (1.0 - std::ldexp(1.0, -20)) / (double)span;
                    run_shape(dtype, nchans, g, t_origin, 0, 1, 0.0, span);
                    run_shape(dtype, nchans, g, t_origin, 1, 1, 0.0, span);
                    run_shape(dtype, nchans, g, t_origin, 3, 10, edge, span);
                    run_shape(dtype, nchans, g, t_origin, 3, 16, 1e-9, span);
                }
    // the last rows the checks admit
    run_shape(RT_DEDISP_U8, 3, 5, (1ull << 31) - 6, 3, 4, 1e-9, (uint64_t)RT_RESAMPLE_MAX_SAMPLES);
}

void run_errors()
{
    const size_t nchans = 5, g = 9;
    Tables T = make_tables(2, nchans, g, 0, 4, 1e-5, 1024);
    const std::vector<uint8_t> canary(g * nchans, 77);
    std::vector<uint8_t> x(canary);
    auto refused = [&](const Tables& B, const char* what, int dtype = RT_DEDISP_U8, uint64_t t_origin = 0) {
        expect(rt_inject_check(dtype, g, nchans, t_origin, B.specs.data(), B.specs.size(), B.tmpl.data(), B.tmpl.size(),
                               B.amp.data(), B.amp.size(), B.delay.data(), B.delay.size()) == RT_EINVAL, what);
        expect(call_host(x.data(), dtype, g, nchans, t_origin, 1, B) == RT_EINVAL, what);
        expect(x == canary, "a refused call wrote nothing");
    };
    expect(rt_inject_check(RT_DEDISP_U8, g, nchans, 0, T.specs.data(), T.specs.size(), T.tmpl.data(), T.tmpl.size(),
                           T.amp.data(), T.amp.size(), T.delay.data(), T.delay.size()) == RT_OK, "baseline");
    Tables B = T;
    B.specs[0].log2bins = 0;
    refused(B, "log2bins 0");
    B = T;
    B.specs[0].log2bins = 17;
    refused(B, "log2bins 17");
    B = T;
    B.specs[1].length = 0;
    refused(B, "length 0");
    B = T;
    B.specs[0].kind = 2;
    refused(B, "kind 2");
    B = T;
    B.specs[0].reserved = 1;
    refused(B, "reserved");
    B = T;
    B.specs[0].span = (uint64_t)RT_RESAMPLE_MAX_SAMPLES + 1;
    B.specs[0].factor = 0.0;
    refused(B, "span above 2^27");
    for (double bad : {std::nan(""), std::numeric_limits<double>::infinity(), 1.0 / 1024.0, -1.0 / 1024.0}) {
        B = T;
        B.specs[1].factor = bad;
        refused(B, "factor refused");
    }
    B = T;
    B.specs[1].factor = std::nextafter(1.0 / 1024.0, 0.0);
    expect(call_host(std::vector<uint8_t>(canary).data(), RT_DEDISP_U8, g, nchans, 0, 1, B) == RT_OK,
           "the largest factor passes");
    B = T;
    B.specs[1].span = 0;
    refused(B, "a factor without a span");
    B = T;
    B.amp[3] = std::numeric_limits<float>::infinity();
    refused(B, "amplitude not finite");
    B = T;
    B.tmpl[B.specs[1].tmpl_off] = std::nanf("");
    refused(B, "template value not finite");
    B = T;
    B.tmpl.pop_back();
    refused(B, "template past tmpl");
    B = T;
    B.amp.pop_back();
    refused(B, "amplitudes past amp");
    B = T;
    B.delay.pop_back();
    refused(B, "delays past delay");
    B = T;
    B.specs[0].amp_off = ~0ull - 1;
    refused(B, "an offset that wraps");
    refused(T, "t_origin + g at 2^31", RT_DEDISP_U8, (1ull << 31) - g);
    refused(T, "a packed type", RT_DEDISP_U4);
    refused(T, "an unknown type", 99);
    expect(rt_inject_host(nullptr, RT_DEDISP_U8, g, nchans, 0, 1, T.specs.data(), T.specs.size(), T.tmpl.data(),
                          T.tmpl.size(), T.amp.data(), T.amp.size(), T.delay.data(), T.delay.size()) == RT_EINVAL,
           "null block");
    expect(rt_inject_host(nullptr, RT_DEDISP_U8, g, nchans, 0, 1, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) == RT_OK,
           "no signals: no pointer is looked at");
}

}  // namespace

int main()
{
    run_shapes();
    run_errors();
    if (g_failed) return 1;
    std::printf("inject_check OK\n");
    return 0;
}
