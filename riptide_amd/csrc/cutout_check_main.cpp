// Host-only checker of the pulse-cutout specification (cutout_host.cpp through
// rt_pulse_cutouts_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a read past the block, the delay table
// or a job's bins is a sanitizer report.  No device call, and none linked.
// Prints "cutout_check OK"; exit status 0 iff every call returned what it
// should and the results agree with a direct recomputation on integer data.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 77;
uint32_t draw(uint32_t n)   // LCG draw in [0, n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_state >> 33) % n);
}

int g_failed = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, rt_last_error());
        g_failed = 1;
    }
}

// channel c of row t of a block of this type, as the value it stands for
double sample(const std::vector<uint8_t>& x, int dtype, size_t nchans, size_t t, size_t c)
{
    const int nbits = dtype == RT_DEDISP_U1 ? 1 : dtype == RT_DEDISP_U2 ? 2 : dtype == RT_DEDISP_U4 ? 4 : 0;
    if (nbits) {
        const uint8_t* row = x.data() + t * (nchans * nbits / 8);
        return (row[c * nbits >> 3] >> (c * nbits & 7)) & ((1u << nbits) - 1u);
    }
    if (dtype == RT_DEDISP_U16) {
        const uint8_t* p = x.data() + (t * nchans + c) * 2;
        return p[0] | p[1] << 8;
    }
    if (dtype == RT_DEDISP_F32) {
        float v;
        std::memcpy(&v, x.data() + (t * nchans + c) * 4, 4);
        return v;
    }
    return dtype == RT_DEDISP_I8 ? (double)(int8_t)x[t * nchans + c] : (double)x[t * nchans + c];
}

// small integer data: every sum is exact in any order, so the plain loops
// below give the specification's bits
void run_type(int dtype, size_t nsamp, size_t nchans, bool masked)
{
    size_t rb = 0;
    expect(rt_dedisp_row_bytes(dtype, nchans, &rb) == RT_OK, "row bytes");
    std::vector<uint8_t> x(nsamp * rb);
    if (dtype == RT_DEDISP_F32) {
        for (size_t i = 0; i < nsamp * nchans; ++i) {
            const float v = (float)((int)draw(17) - 8);
            std::memcpy(x.data() + 4 * i, &v, 4);
        }
    } else {
        for (auto& b : x) b = (uint8_t)draw(256);
        if (dtype == RT_DEDISP_U16)
            for (size_t i = 0; i < nsamp * nchans; ++i) x[2 * i + 1] &= 0x03;   // below 1024: float sums stay exact
    }
    const size_t R = 3;
    const int64_t max_delay = 40;
    std::vector<int32_t> delays(R * nchans);
    for (auto& d : delays) d = (int32_t)draw(60) - 10;   // some below 0, some above max_delay: clamped
    std::vector<uint8_t> mask(nchans);
    for (auto& m : mask) m = masked && draw(4) == 0;
    const uint32_t C = (uint32_t)nchans;
    const int64_t N = (int64_t)nsamp;
    std::vector<rt_cutout_spec> jobs = {
        {0, 0, 1, 16, 0, 0, C, 0},                          // the whole band, no decimation
        {-37, 0, 3, 33, 1, 0, C, 0},                        // starts before the block
        {N - 50, 0, 7, 20, 2, 0, C, 0},                     // runs past its end
        {N + 5, 0, 2, 9, 0, 0, C, 0},                       // wholly behind it
        {-1000, 0, 5, 10, 1, 0, C, 0},                      // wholly in front of it
        {N - 45, 0, 1, 8, 2, 0, C, 0},                      // start + delay crosses the end for some channels
        {10, 0, 4, 5, 0, C / 2, C / 2, 0},                  // an empty band
        {10, 0, 4, 5, 1, C / 3, C, 0},                      // a band
        {-5, 0, (uint32_t)nsamp + 9, 2, 2, 0, C, 0},        // a bin longer than the block
        {3, 0, 300, 1, 0, 1 % C, C, 0},                     // one long bin
    };
    size_t total = 0;
    for (auto& j : jobs) {
        j.out_off = total;
        total += j.nbins;
    }
    std::vector<float> out(total, -1.0f);
    expect(rt_pulse_cutouts_host(x.data(), dtype, nsamp, nchans, delays.data(), R, max_delay,
                                 masked ? mask.data() : nullptr, jobs.data(), jobs.size(), out.data(), total, 0u,
                                 nullptr) == RT_OK, "rt_pulse_cutouts_host");
    for (const auto& j : jobs)
        for (uint32_t n = 0; n < j.nbins; ++n) {
            double acc = 0.0;
            for (uint32_t c = j.band_lo; c < j.band_hi; ++c) {
                if (masked && mask[c]) continue;
                const int64_t d = std::min<int64_t>(std::max<int64_t>(delays[j.delay_row * nchans + c], 0), max_delay);
                for (uint32_t k = 0; k < j.factor; ++k) {
                    const int64_t t = j.start + (int64_t)n * j.factor + k + d;
                    if (t >= 0 && t < N) acc += sample(x, dtype, nchans, (size_t)t, c);
                }
            }
            if (out[j.out_off + n] != (float)acc) {
                std::printf("FAILED: type %d bin %u of the job at %lld\n", dtype, n, (long long)j.start);
                g_failed = 1;
                return;
            }
        }
    // the zero-DM filter and a block mask: the call runs on exact-size arrays
    // (its values are pinned to numpy by the tests)
    std::vector<uint8_t> cells(((nsamp + 7 + 12) / 13) * nchans);
    for (auto& b : cells) b = draw(5) == 0;
    std::vector<uint8_t> fill(nchans * 4, 1);
    if (dtype == RT_DEDISP_F32)
        for (size_t c = 0; c < nchans; ++c) {
            const float v = 2.0f;
            std::memcpy(fill.data() + 4 * c, &v, 4);
        }
    rt_block_mask bm{cells.data(), cells.size() / nchans, 13, 7, fill.data()};
    expect(rt_pulse_cutouts_host(x.data(), dtype, nsamp, nchans, delays.data(), R, max_delay, mask.data(),
                                 jobs.data(), jobs.size(), out.data(), total, RT_DEDISP_ZERO_DM, &bm) == RT_OK,
           "zero-DM with a block mask");
}

void run_errors()
{
    std::vector<uint8_t> x(64 * 8, 1);
    std::vector<int32_t> delays(2 * 8, 0);
    std::vector<float> out(32);
    auto call = [&](rt_cutout_spec j, int dtype = RT_DEDISP_U8, size_t R = 2, int64_t md = 10, uint32_t flags = 0u) {
        return rt_pulse_cutouts_host(x.data(), dtype, 64, 8, delays.data(), R, md, nullptr, &j, 1, out.data(),
                                     out.size(), flags, nullptr);
    };
    expect(call({0, 0, 2, 32, 1, 0, 8, 0}) == RT_OK, "baseline");
    expect(call({0, 0, 0, 32, 1, 0, 8, 0}) == RT_EINVAL, "factor 0");
    expect(call({0, 0, 2, 0, 1, 0, 8, 0}) == RT_EINVAL, "no bins");
    expect(call({0, 0, 2, 32, 2, 0, 8, 0}) == RT_EINVAL, "delay row past the table");
    expect(call({0, 0, 2, 32, 1, 5, 4, 0}) == RT_EINVAL, "band lo > hi");
    expect(call({0, 0, 2, 32, 1, 0, 9, 0}) == RT_EINVAL, "band past nchans");
    expect(call({0, 1, 2, 32, 1, 0, 8, 0}) == RT_EINVAL, "bins past out");
    expect(call({0, 0, 1u << 20, 1, 1, 0, 8, 0}) == RT_OK, "8 x 2^20 x 255 is below 2^31");
    expect(call({0, 0, 1u << 21, 1, 1, 0, 8, 0}) == RT_EINVAL, "8 x 2^21 x 255 is not");
    expect(call({0, 0, 1u << 21, 1, 1, 0, 8, 0}, RT_DEDISP_U8, 2, 10, RT_DEDISP_ZERO_DM) == RT_OK,
           "a float sum has no such limit");
    expect(call({0, 0, 1u << 30, 2, 1, 0, 0, 0}) == RT_EINVAL, "window of 2^31 samples");
    expect(call({(int64_t)1 << 41, 0, 1, 1, 1, 0, 8, 0}) == RT_EINVAL, "start above 2^40");
    expect(call({0, 0, 2, 32, 1, 0, 8, 0}, 77) == RT_EINVAL, "unknown type");
    expect(call({0, 0, 2, 32, 1, 0, 8, 0}, RT_DEDISP_U8, 0) == RT_EINVAL, "no delay rows");
    expect(call({0, 0, 2, 32, 1, 0, 8, 0}, RT_DEDISP_U8, 2, -1) == RT_EINVAL, "negative max_delay");
    expect(call({0, 0, 2, 32, 1, 0, 8, 0}, RT_DEDISP_U8, 2, 10, 2u) == RT_EINVAL, "unknown flag");
    expect(rt_pulse_cutouts_host(x.data(), RT_DEDISP_U8, 64, 8, delays.data(), 2, 10, nullptr, nullptr, 0, nullptr, 0,
                                 0u, nullptr) == RT_OK, "no jobs");
    size_t tile = 0, ndw = 0;
    int staged = -1;
    expect(rt_pulse_cutouts_plan(1, 0, 4096, &tile, &ndw, &staged) == RT_OK && tile >= 64 && ndw == 1024 && staged == 1,
           "plan: 4096 aligned bytes");
    expect(rt_pulse_cutouts_plan(1, 1, 4097, &tile, &ndw, &staged) == RT_OK && ndw == 1025 && staged == 0,
           "plan: 4096 bytes from byte 1");
    expect(rt_pulse_cutouts_plan(4, 5, 1029, nullptr, &ndw, &staged) == RT_OK && ndw == 1024 && staged == 1,
           "plan: 1024 floats");
    expect(rt_pulse_cutouts_plan(2, 0, 4, nullptr, nullptr, nullptr) == RT_EINVAL, "plan: esize");
    expect(rt_pulse_cutouts_plan(1, 4, 4, nullptr, nullptr, nullptr) == RT_EINVAL, "plan: empty span");
}

}  // namespace

int main()
{
    const int types[] = {RT_DEDISP_U8, RT_DEDISP_I8, RT_DEDISP_F32, RT_DEDISP_U1, RT_DEDISP_U2, RT_DEDISP_U4,
                         RT_DEDISP_U16};
    for (int dtype : types) {
        run_type(dtype, 200, 8, false);
        run_type(dtype, 333, 24, true);
    }
    run_type(RT_DEDISP_U8, 1, 1, false);   // one sample, one channel
    run_errors();
    if (g_failed) return 1;
    std::printf("cutout_check OK\n");
    return 0;
}
