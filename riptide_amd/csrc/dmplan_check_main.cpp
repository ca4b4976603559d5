// Host sanitizer checker of the DM plan (`make asan`: g++, AddressSanitizer +
// UBSan, no HIP): rt_dm_plan, rt_dedisperse_ds_host and rt_dedisperse_steps_check
// on exact-size heap arrays, so that a read or write one element past any of
// them is an error, at the edge shapes of tests/test_dmplan_host.py and
// tests/test_gpu_dmplan.py; every refusal must come back as RT_EINVAL.
// Prints "dmplan_check OK".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "riptide_amd.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, rt_last_error()); \
            ++failures;                                                              \
        }                                                                            \
    } while (0)

constexpr double kKdm = 1.0 / 2.41e-4;

template <class T>
std::unique_ptr<T[]> exact(size_t n)
{
    return std::unique_ptr<T[]>(new T[n ? n : 1]);
}

uint32_t lcg(uint32_t& s)
{
    s = s * 1664525u + 1013904223u;
    return s >> 8;
}

// the planner: count, then fill exact-size arrays; the rule of the trials and of the factors
void check_plan(size_t nchans, double f_hi, double f_lo, double tsamp, double dm_min, double dm_max, double wmin,
                double oversample, uint32_t max_downsamp, bool ascending)
{
    auto freqs = exact<double>(nchans);
    for (size_t c = 0; c < nchans; ++c) {
        const double f = f_hi - (f_hi - f_lo) * (double)c / (double)(nchans - 1);
        freqs[ascending ? nchans - 1 - c : c] = f;
    }
    size_t n = 0;
    CHECK(rt_dm_plan(freqs.get(), nchans, tsamp, dm_min, dm_max, wmin, oversample, max_downsamp, kKdm, nullptr,
                     nullptr, 0, &n) == RT_OK);
    CHECK(n >= 1);
    auto dms = exact<double>(n);
    auto fs = exact<uint32_t>(n);
    size_t m = 0;
    CHECK(rt_dm_plan(freqs.get(), nchans, tsamp, dm_min, dm_max, wmin, oversample, max_downsamp, kKdm, dms.get(),
                     fs.get(), n, &m) == RT_OK);
    CHECK(m == n && dms[0] == dm_min);
    for (size_t i = 1; i < n; ++i) CHECK(dms[i] > dms[i - 1] && fs[i] >= fs[i - 1]);
    for (size_t i = 0; i < n; ++i) CHECK(fs[i] >= 1 && fs[i] <= max_downsamp && (fs[i] & (fs[i] - 1)) == 0);
    if (n > 1)   // one short: refused, nothing written past the capacity
        CHECK(rt_dm_plan(freqs.get(), nchans, tsamp, dm_min, dm_max, wmin, oversample, max_downsamp, kKdm, dms.get(),
                         fs.get(), n - 1, &m) == RT_EINVAL);
}

void check_plan_refusals()
{
    const double two[2] = {400.0, 380.0};
    const double bad[2] = {400.0, -1.0};
    const double same[2] = {400.0, 400.0};
    size_t n = 0;
    double dm;
    uint32_t f;
    CHECK(rt_dm_plan(two, 1, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(bad, 2, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(same, 2, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 0.0, 0, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, -1, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 20, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, INFINITY, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, NAN, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 0, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 0, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 257, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 64, 0.0, nullptr, nullptr, 0, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, &dm, nullptr, 1, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, nullptr, &f, 1, &n) == RT_EINVAL);
    CHECK(rt_dm_plan(two, 2, 1e-3, 0, 10, 1e-3, 2, 64, kKdm, nullptr, nullptr, 0, nullptr) == RT_EINVAL);
    {   // more than 2^20 trials: 2^20 channels of 368-400 MHz, a microsecond wide pulse, DM up to 1000
        const size_t nch = (size_t)1 << 20;
        auto fine = exact<double>(nch);
        for (size_t c = 0; c < nch; ++c) fine[c] = 400.0 - 32.0 * (double)c / (double)(nch - 1);
        CHECK(rt_dm_plan(fine.get(), nch, 1e-3, 0, 1000, 1e-6, 2, 64, kKdm, nullptr, nullptr, 0, &n) == RT_EINVAL);
    }
    CHECK(rt_dm_plan(two, 2, 1e-3, 5, 5, 1e-3, 2, 64, kKdm, &dm, &f, 1, &n) == RT_OK && n == 1 && dm == 5.0);
}

// the specification at one shape: every array exactly as long as it is read or written
void check_ds(int dtype, size_t nsamp, size_t nchans, size_t f, size_t ndm, uint32_t flags, bool masked, bool cells)
{
    size_t rb = 0;
    CHECK(rt_dedisp_row_bytes(dtype, nchans, &rb) == RT_OK);
    uint32_t seed = (uint32_t)(nsamp * 31 + nchans * 7 + f);
    auto x = exact<uint8_t>(nsamp * rb);
    for (size_t i = 0; i < nsamp * rb; ++i) x[i] = (uint8_t)lcg(seed);
    if (dtype == RT_DEDISP_F32) {
        float* xf = reinterpret_cast<float*>(x.get());
        for (size_t i = 0; i < nsamp * nchans; ++i) xf[i] = (float)((int)(lcg(seed) % 2001) - 1000) * 0.01f;
    }
    const size_t nz = nsamp / f;
    const int64_t md = (int64_t)(nz / 3);
    auto delays = exact<int64_t>(ndm * nchans);
    for (size_t i = 0; i < ndm * nchans; ++i) delays[i] = (int64_t)(lcg(seed) % (uint32_t)(md + 1));
    delays[ndm * nchans - 1] = md;
    auto mask = exact<uint8_t>(nchans);
    for (size_t c = 0; c < nchans; ++c) mask[c] = c % 3 == 1;
    const size_t block_len = 37, t_origin = 5 * f;
    const size_t nblocks = (t_origin + nsamp + block_len - 1) / block_len;
    auto flags_c = exact<uint8_t>(nblocks * nchans);
    for (size_t i = 0; i < nblocks * nchans; ++i) flags_c[i] = lcg(seed) % 5 == 0;
    const size_t fill_bytes = dtype == RT_DEDISP_F32 ? 4 : dtype == RT_DEDISP_U16 ? 2 : 1;
    auto fill = exact<uint8_t>(nchans * fill_bytes);
    for (size_t i = 0; i < nchans * fill_bytes; ++i) fill[i] = dtype == RT_DEDISP_F32 ? 0 : (uint8_t)lcg(seed);
    rt_block_mask bm{flags_c.get(), nblocks, block_len, t_origin, fill.get()};
    const size_t nout = nz - (size_t)md;
    auto out = exact<float>(ndm * nout);
    CHECK(rt_dedisperse_ds_host(x.get(), dtype, nsamp, nchans, delays.get(), masked ? mask.get() : nullptr, ndm, md, f,
                                nout, out.get(), flags, cells ? &bm : nullptr) == RT_OK);
    for (size_t i = 0; i < ndm * nout; ++i) CHECK(std::isfinite(out[i]));
    // one output too many, a delay past max_delay, a mask origin off the decimated grid
    CHECK(rt_dedisperse_ds_host(x.get(), dtype, nsamp, nchans, delays.get(), nullptr, ndm, md, f, nout + 1, out.get(),
                                flags, nullptr) == RT_EINVAL);
    if (md > 0)
        CHECK(rt_dedisperse_ds_host(x.get(), dtype, nsamp, nchans, delays.get(), nullptr, ndm, md - 1, f, 1,
                                    out.get(), flags, nullptr) == RT_EINVAL);
    if (f > 1) {
        bm.t_origin = t_origin + 1;
        CHECK(rt_dedisperse_ds_host(x.get(), dtype, nsamp, nchans, delays.get(), nullptr, ndm, md, f, nout, out.get(),
                                    flags, &bm) == RT_EINVAL);
    }
}

void check_ds_refusals()
{
    const size_t f = 256;
    auto x = exact<uint8_t>(2 * f * 258);
    for (size_t i = 0; i < 2 * f * 258; ++i) x[i] = 255;
    auto delays = exact<int64_t>(258);
    for (size_t c = 0; c < 258; ++c) delays[c] = 0;
    float out[2];
    // the exactness cap: 255 * 256 * 257 < 2^24 <= 255 * 256 * 258
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 257, delays.get(), nullptr, 1, 0, f, 2, out, 0,
                                nullptr) == RT_OK);
    CHECK(out[0] == 255.0f * 256 * 257 && out[1] == out[0]);
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 258, delays.get(), nullptr, 1, 0, f, 2, out, 0,
                                nullptr) == RT_EINVAL);
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 258, delays.get(), nullptr, 1, 0, f, 2, out,
                                RT_DEDISP_ZERO_DM, nullptr) == RT_OK);
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 4, delays.get(), nullptr, 1, 0, 0, 2, out, 0,
                                nullptr) == RT_EINVAL);
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 4, delays.get(), nullptr, 1, 0, 257, 1, out, 0,
                                nullptr) == RT_EINVAL);
    CHECK(rt_dedisperse_ds_host(x.get(), 77, 2 * f, 4, delays.get(), nullptr, 1, 0, 2, 1, out, 0, nullptr) ==
          RT_EINVAL);
    CHECK(rt_dedisperse_ds_host(x.get(), RT_DEDISP_U8, 2 * f, 4, delays.get(), nullptr, 1, 0, 2, 1, out, 2u,
                                nullptr) == RT_EINVAL);
}

// the step table: exact-size tables, every refusal
void check_steps()
{
    const size_t nsamp = 1000, nchans = 16;
    auto good = [] {
        rt_dedisp_step s{};
        s.out_stride = 240;
        s.ndm = 3;
        s.max_delay = 10;
        s.downsamp = 4;
        return s;
    };
    auto run = [&](const rt_dedisp_step& s, int dtype = RT_DEDISP_U8, const rt_block_mask* bm = nullptr) {
        auto t = exact<rt_dedisp_step>(1);
        t[0] = s;
        return rt_dedisperse_steps_check(dtype, nsamp, nchans, t.get(), 1, 48, 720, 0, bm);
    };
    CHECK(run(good()) == RT_OK);
    rt_dedisp_step s = good();
    s.downsamp = 0;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.downsamp = 257;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.max_delay = 250;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.reserved = 1;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.ndm = 0;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.delays_off = 1;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.delays_off = ~0ull;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.out_stride = 239;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.out_off = 1;
    CHECK(run(s) == RT_EINVAL);
    s = good();
    s.out_off = ~0ull;
    s.out_stride = ~0ull;
    CHECK(run(s) == RT_EINVAL);
    CHECK(run(good(), 77) == RT_EINVAL);
    auto cells = exact<uint8_t>(28 * nchans);
    auto fill = exact<uint8_t>(nchans);
    rt_block_mask bm{cells.get(), 28, 37, 8, fill.get()};
    CHECK(run(good(), RT_DEDISP_U8, &bm) == RT_OK);
    bm.t_origin = 6;
    CHECK(run(good(), RT_DEDISP_U8, &bm) == RT_EINVAL);
    bm.t_origin = 40;   // the rows reach past the cells
    CHECK(run(good(), RT_DEDISP_U8, &bm) == RT_EINVAL);
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U8, nsamp, nchans, nullptr, 0, 48, 720, 0, nullptr) == RT_EINVAL);
    // three steps of one table, the second's cap: 255 * 256 * 258 >= 2^24
    auto t = exact<rt_dedisp_step>(3);
    for (int k = 0; k < 3; ++k) {
        t[k] = rt_dedisp_step{};
        t[k].ndm = 1;
        t[k].downsamp = k == 1 ? 256 : 1;
        t[k].out_stride = 1000;
        t[k].out_off = 1000 * (uint64_t)k;
    }
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U8, nsamp, 257, t.get(), 3, 257, 3000, 0, nullptr) == RT_OK);
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U8, nsamp, 258, t.get(), 3, 258, 3000, 0, nullptr) == RT_EINVAL);
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U8, nsamp, 258, t.get(), 3, 258, 3000, RT_DEDISP_ZERO_DM, nullptr) ==
          RT_OK);
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U2, nsamp, 258, t.get(), 3, 258, 3000, 0, nullptr) == RT_EINVAL);   // bytes
    CHECK(rt_dedisperse_steps_check(RT_DEDISP_U2, nsamp, 256, t.get(), 3, 256, 3000, 0, nullptr) == RT_OK);
}

}  // namespace

int main()
{
    check_plan(1024, 1600.0, 1200.4, 64e-6, 0.0, 1000.0, 1e-3, 2.0, 64, false);
    check_plan(4096, 400.0, 300.0, 256e-6, 12.5, 300.0, 1e-3, 1.0, 8, true);
    check_plan(2, 400.0, 380.0, 1e-3, 0.0, 2000.0, 1e-3, 3.5, 256, false);
    check_plan(16, 400.0, 368.0, 1e-3, 0.0, 0.0, 1e-3, 2.0, 1, false);
    check_plan_refusals();
    const int types[] = {RT_DEDISP_U8, RT_DEDISP_I8, RT_DEDISP_F32, RT_DEDISP_U1, RT_DEDISP_U2, RT_DEDISP_U4,
                         RT_DEDISP_U16};
    const size_t sizes[] = {97, 1000, 1003};
    const size_t factors[] = {1, 2, 3, 4, 5, 8, 37};
    int k = 0;
    for (int dtype : types)
        for (size_t nsamp : sizes)
            for (size_t f : factors) {
                if (nsamp / f < 2) continue;
                ++k;
                check_ds(dtype, nsamp, k % 2 ? 72 : 8, f, 1 + k % 3, k % 4 < 2 ? 0u : RT_DEDISP_ZERO_DM, k % 3 == 0,
                         k % 5 < 2);
            }
    check_ds(RT_DEDISP_U8, 600, 2, 256, 2, 0, false, true);
    check_ds_refusals();
    check_steps();
    if (failures) {
        std::printf("dmplan_check: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("dmplan_check OK\n");
    return 0;
}
