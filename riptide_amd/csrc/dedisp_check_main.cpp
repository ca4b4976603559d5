// Host-only checker of the dedispersion delay table and specification
// (rt_dedisperse_delays, rt_dedisperse_host, and the zero-DM and channel
// statistics forms rt_dedisperse_host_opt, rt_zero_dm_mean_host,
// rt_channel_stats_host: dedisp_host.cpp), built with
// AddressSanitizer + UBSan by `make -C riptide_amd/csrc asan`.  Every array is
// a heap block of exactly the size the entry point may touch, so a read past
// the last sample, a delay row or the mask is a sanitizer report.  No device
// call, and none linked.  Usage:
//   dedisp_check
// Runs the edge shapes (1, 3, 37, 64, 65 channels, both band orders, DM 0,
// nout = nsamp - max_delay and nout = 1, with and without a mask, the three
// sample types) against a recount, the same shapes with RT_DEDISP_ZERO_DM
// and through the statistics, the packed sample types (1, 2, 4 and 16 bit:
// whole-byte rows of 1 to 18 bytes, blocks that end on the array's last byte),
// then every error return, and the staging rule's table and refusals
// (rt_dedisperse_span_plan).  Exit status 0 iff all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "riptide_amd.h"

namespace {

uint64_t g_state = 12345;
uint32_t draw()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

int fails = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, rt_last_error());
        ++fails;
    }
}

template <class T>
double sample(const std::vector<unsigned char>& x, size_t i)
{
    T v;
    std::memcpy(&v, x.data() + i * sizeof(T), sizeof(T));
    return (double)v;
}

void run_shape(size_t nchans, bool ascending, int dtype, bool masked, bool single_out)
{
    const double tsamp = 1e-3, kdm = 1.0 / 2.41e-4;
    const double dms_[] = {0.0, 50.0, 12.5, 50.0, 3.0};
    const size_t ndm = 5;
    std::vector<double> freqs(nchans), dms(dms_, dms_ + ndm);
    for (size_t c = 0; c < nchans; ++c) {
        const double step = 32.0 / (double)nchans;
        freqs[c] = ascending ? 368.0 + step * (double)c : 400.0 - step * (double)c;
    }
    std::vector<int64_t> delays(ndm * nchans);
    int64_t max_delay = -1;
    expect(rt_dedisperse_delays(freqs.data(), nchans, dms.data(), ndm, tsamp, kdm, delays.data(), &max_delay) == RT_OK,
           "delays");
    for (size_t c = 0; c < nchans; ++c) expect(delays[c] == 0, "DM 0 has zero delays");
    int64_t recount = 0;
    for (int64_t v : delays) recount = v > recount ? v : recount;
    expect(recount == max_delay, "max_delay");
    const size_t nsamp = (size_t)max_delay + 300;
    const size_t nout = single_out ? 1 : nsamp - (size_t)max_delay;
    const size_t esize = dtype == RT_DEDISP_F32 ? 4 : 1;
    std::vector<unsigned char> x(nsamp * nchans * esize);
    for (size_t i = 0; i < nsamp * nchans; ++i) {
        if (dtype == RT_DEDISP_F32) {
            const float v = (float)((double)draw() / 4294967296.0 - 0.5);
            std::memcpy(x.data() + 4 * i, &v, 4);
        } else {
            x[i] = (unsigned char)draw();
        }
    }
    std::vector<uint8_t> mask;
    if (masked) {
        mask.assign(nchans, 0);
        mask[0] = 1;
        mask[nchans - 1] = 1;
        if (nchans > 4) mask[nchans / 2] = 1;
    }
    std::vector<float> out(ndm * nout);
    expect(rt_dedisperse_host(x.data(), dtype, nsamp, nchans, delays.data(), masked ? mask.data() : nullptr, ndm,
                              max_delay, nout, out.data()) == RT_OK,
           "dedisperse_host");
    for (size_t d = 0; d < ndm; ++d)
        for (size_t t = 0; t < nout; ++t) {
            double ref = 0.0, mag = 0.0;
            for (size_t c = 0; c < nchans; ++c) {
                if (masked && mask[c]) continue;
                const size_t i = (t + (size_t)delays[d * nchans + c]) * nchans + c;
                const double v = dtype == RT_DEDISP_U8 ? sample<uint8_t>(x, i)
                                 : dtype == RT_DEDISP_I8 ? sample<int8_t>(x, i) : sample<float>(x, i);
                ref += v;
                mag += std::fabs(v);
            }
            const double tol = dtype == RT_DEDISP_F32 ? (double)nchans * std::ldexp(1.0, -24) * mag : 0.0;
            if (std::fabs((double)out[d * nout + t] - ref) > tol) {
                std::printf("FAILED: nchans %zu dtype %d dm %zu t %zu: %g vs %g\n", nchans, dtype, d, t,
                            (double)out[d * nout + t], ref);
                ++fails;
                return;
            }
        }
}

// The same shape through rt_zero_dm_mean_host, rt_dedisperse_host_opt with
// RT_DEDISP_ZERO_DM and rt_channel_stats_host (in two halves), every array of
// exact size.
void run_rfi_shape(size_t nchans, int dtype, bool masked, bool single_out)
{
    const double tsamp = 1e-3, kdm = 1.0 / 2.41e-4;
    const size_t ndm = 5;
    std::vector<double> freqs(nchans), dms{0.0, 50.0, 12.5, 50.0, 3.0};
    for (size_t c = 0; c < nchans; ++c) freqs[c] = 400.0 - 32.0 / (double)nchans * (double)c;
    std::vector<int64_t> delays(ndm * nchans);
    int64_t max_delay = -1;
    expect(rt_dedisperse_delays(freqs.data(), nchans, dms.data(), ndm, tsamp, kdm, delays.data(), &max_delay) == RT_OK,
           "delays");
    const size_t nsamp = (size_t)max_delay + 300;
    const size_t nout = single_out ? 1 : nsamp - (size_t)max_delay;
    const size_t esize = dtype == RT_DEDISP_F32 ? 4 : 1;
    std::vector<unsigned char> x(nsamp * nchans * esize);
    for (size_t i = 0; i < nsamp * nchans; ++i) {
        if (dtype == RT_DEDISP_F32) {
            const float v = (float)((double)draw() / 4294967296.0 - 0.5);
            std::memcpy(x.data() + 4 * i, &v, 4);
        } else {
            x[i] = (unsigned char)draw();
        }
    }
    auto value = [&](size_t i) {
        return dtype == RT_DEDISP_U8 ? sample<uint8_t>(x, i) : dtype == RT_DEDISP_I8 ? sample<int8_t>(x, i)
                                                                                      : sample<float>(x, i);
    };
    std::vector<uint8_t> mask;
    if (masked) {
        mask.assign(nchans, 0);
        mask[0] = 1;
        mask[nchans - 1] = 1;
    }
    const uint8_t* mk = masked ? mask.data() : nullptr;
    size_t nu = 0;
    for (size_t c = 0; c < nchans; ++c) nu += !masked || !mask[c];

    std::vector<float> m(nsamp);
    expect(rt_zero_dm_mean_host(x.data(), dtype, nsamp, nchans, mk, m.data()) == RT_OK, "zero_dm_mean_host");
    for (size_t t = 0; t < nsamp; ++t) {
        double s = 0.0;
        for (size_t c = 0; c < nchans; ++c)
            if (!masked || !mask[c]) s += value(t * nchans + c);
        const float want = nu ? (float)(s / (double)nu) : 0.0f;
        // 8-bit: s is an exact integer, so the mean is the same bits
        const double tol = dtype == RT_DEDISP_F32 ? std::ldexp(std::fabs((double)want), -23) : 0.0;
        if (std::fabs((double)m[t] - (double)want) > tol) {
            std::printf("FAILED: zero-DM mean nchans %zu dtype %d t %zu: %g vs %g\n", nchans, dtype, t, (double)m[t],
                        (double)want);
            ++fails;
            return;
        }
    }

    std::vector<float> out(ndm * nout);
    expect(rt_dedisperse_host_opt(x.data(), dtype, nsamp, nchans, delays.data(), mk, ndm, max_delay, nout, out.data(),
                                  RT_DEDISP_ZERO_DM) == RT_OK,
           "dedisperse_host_opt");
    for (size_t d = 0; d < ndm; ++d)
        for (size_t t = 0; t < nout; ++t) {
            double ref = 0.0, mag = 0.0;
            for (size_t c = 0; c < nchans; ++c) {
                if (masked && mask[c]) continue;
                const size_t tt = t + (size_t)delays[d * nchans + c];
                const double y = value(tt * nchans + c) - (double)m[tt];
                ref += y;
                mag += std::fabs(y);
            }
            const double tol = (double)(nchans + 2) * std::ldexp(1.0, -24) * mag;
            if (std::fabs((double)out[d * nout + t] - ref) > tol) {
                std::printf("FAILED: zero-DM nchans %zu dtype %d dm %zu t %zu: %g vs %g\n", nchans, dtype, d, t,
                            (double)out[d * nout + t], ref);
                ++fails;
                return;
            }
        }

    // the plain call through the flag-taking form
    std::vector<float> plain(ndm * nout), plain_opt(ndm * nout);
    expect(rt_dedisperse_host(x.data(), dtype, nsamp, nchans, delays.data(), mk, ndm, max_delay, nout,
                              plain.data()) == RT_OK, "dedisperse_host");
    expect(rt_dedisperse_host_opt(x.data(), dtype, nsamp, nchans, delays.data(), mk, ndm, max_delay, nout,
                                  plain_opt.data(), 0u) == RT_OK, "dedisperse_host_opt, flags 0");
    expect(std::memcmp(plain.data(), plain_opt.data(), plain.size() * sizeof(float)) == 0,
           "flags 0 equals the plain call");

    // the statistics: two halves, each an exact-size copy, into one accumulator
    std::vector<double> acc(2 * nchans, 0.0);
    const size_t half = nsamp / 3;
    std::vector<unsigned char> a(x.begin(), x.begin() + (std::ptrdiff_t)(half * nchans * esize));
    std::vector<unsigned char> b(x.begin() + (std::ptrdiff_t)(half * nchans * esize), x.end());
    expect(rt_channel_stats_host(a.data(), dtype, half, nchans, acc.data()) == RT_OK, "channel_stats_host (a)");
    expect(rt_channel_stats_host(b.data(), dtype, nsamp - half, nchans, acc.data()) == RT_OK,
           "channel_stats_host (b)");
    for (size_t c = 0; c < nchans; ++c) {
        double s = 0.0, q = 0.0, sa = 0.0;
        for (size_t t = 0; t < nsamp; ++t) {
            const double v = value(t * nchans + c);
            s += v;
            q += v * v;
            sa += std::fabs(v);
        }
        const double u = dtype == RT_DEDISP_F32 ? 2.0 * (double)nsamp * std::ldexp(1.0, -53) : 0.0;
        if (std::fabs(acc[c] - s) > u * sa || std::fabs(acc[nchans + c] - q) > u * q) {
            std::printf("FAILED: channel stats nchans %zu dtype %d channel %zu\n", nchans, dtype, c);
            ++fails;
            return;
        }
    }
}

// Packed sample types: a block of exactly nsamp * row_bytes heap bytes (the
// last row ends on the array's last byte) through the plain sum, the zero-DM
// form, the mean series and the statistics, against a restatement that
// extracts the bits sample by sample.
void run_packed_shape(int nbits, size_t nchans, bool masked)
{
    const int dtype = 0x100 + nbits;
    const double tsamp = 1e-3, kdm = 1.0 / 2.41e-4;
    const size_t ndm = 3;
    std::vector<double> freqs(nchans), dms{0.0, 50.0, 12.5};
    for (size_t c = 0; c < nchans; ++c) freqs[c] = 400.0 - 32.0 / (double)nchans * (double)c;
    std::vector<int64_t> delays(ndm * nchans);
    int64_t max_delay = -1;
    expect(rt_dedisperse_delays(freqs.data(), nchans, dms.data(), ndm, tsamp, kdm, delays.data(), &max_delay) == RT_OK,
           "delays");
    const size_t nsamp = (size_t)max_delay + 41, nout = nsamp - (size_t)max_delay;
    size_t rb = 0;
    expect(rt_dedisp_row_bytes(dtype, nchans, &rb) == RT_OK && rb == nchans * (size_t)nbits / 8, "row_bytes");
    std::vector<unsigned char> x(nsamp * rb);
    for (unsigned char& b : x) b = (unsigned char)draw();
    // the restatement: bit k of the row, counted from the least significant
    // bit of its first byte (16 bit: the same, bytes little-endian)
    auto value = [&](size_t t, size_t c) {
        double v = 0.0;
        for (int k = 0; k < nbits; ++k) {
            const size_t bit = c * (size_t)nbits + (size_t)k;
            if (x[t * rb + bit / 8] >> (bit % 8) & 1) v += std::ldexp(1.0, k);
        }
        return v;
    };
    std::vector<uint8_t> mask;
    if (masked) {
        mask.assign(nchans, 0);
        mask[0] = 1;
        mask[nchans - 1] = 1;
    }
    const uint8_t* mk = masked ? mask.data() : nullptr;
    size_t nu = 0;
    for (size_t c = 0; c < nchans; ++c) nu += !masked || !mask[c];

    std::vector<float> out(ndm * nout), m(nsamp);
    expect(rt_dedisperse_host(x.data(), dtype, nsamp, nchans, delays.data(), mk, ndm, max_delay, nout, out.data()) ==
               RT_OK, "dedisperse_host (packed)");
    expect(rt_zero_dm_mean_host(x.data(), dtype, nsamp, nchans, mk, m.data()) == RT_OK, "zero_dm_mean_host (packed)");
    for (size_t t = 0; t < nsamp; ++t) {
        double s = 0.0;
        for (size_t c = 0; c < nchans; ++c)
            if (!masked || !mask[c]) s += value(t, c);
        const float want = nu ? (float)(s / (double)nu) : 0.0f;
        if (m[t] != want) {   // s is an exact integer: the same bits
            std::printf("FAILED: packed mean nbits %d nchans %zu t %zu: %g vs %g\n", nbits, nchans, t, (double)m[t],
                        (double)want);
            ++fails;
            return;
        }
    }
    std::vector<float> zout(ndm * nout);
    expect(rt_dedisperse_host_opt(x.data(), dtype, nsamp, nchans, delays.data(), mk, ndm, max_delay, nout, zout.data(),
                                  RT_DEDISP_ZERO_DM) == RT_OK, "dedisperse_host_opt (packed, zero-DM)");
    for (size_t d = 0; d < ndm; ++d)
        for (size_t t = 0; t < nout; ++t) {
            double ref = 0.0, mag = 0.0, zref = 0.0, zmag = 0.0;
            for (size_t c = 0; c < nchans; ++c) {
                if (masked && mask[c]) continue;
                const size_t tt = t + (size_t)delays[d * nchans + c];
                const double v = value(tt, c), y = v - (double)m[tt];
                ref += v;
                mag += v;
                zref += y;
                zmag += std::fabs(y);
            }
            // 1/2/4 bit: exact integers; 16 bit: float32 additions in channel order
            const double tol = nbits == 16 ? (double)nchans * std::ldexp(1.0, -24) * mag : 0.0;
            const double ztol = (double)(nchans + 2) * std::ldexp(1.0, -24) * zmag;
            if (std::fabs((double)out[d * nout + t] - ref) > tol ||
                std::fabs((double)zout[d * nout + t] - zref) > ztol) {
                std::printf("FAILED: packed nbits %d nchans %zu dm %zu t %zu: %g vs %g, zero-DM %g vs %g\n", nbits,
                            nchans, d, t, (double)out[d * nout + t], ref, (double)zout[d * nout + t], zref);
                ++fails;
                return;
            }
        }
    std::vector<double> acc(2 * nchans, 0.0);
    const size_t half = nsamp / 3;
    std::vector<unsigned char> a(x.begin(), x.begin() + (std::ptrdiff_t)(half * rb));
    std::vector<unsigned char> b(x.begin() + (std::ptrdiff_t)(half * rb), x.end());
    expect(rt_channel_stats_host(a.data(), dtype, half, nchans, acc.data()) == RT_OK, "channel_stats_host (packed a)");
    expect(rt_channel_stats_host(b.data(), dtype, nsamp - half, nchans, acc.data()) == RT_OK,
           "channel_stats_host (packed b)");
    for (size_t c = 0; c < nchans; ++c) {
        double s = 0.0, q = 0.0;
        for (size_t t = 0; t < nsamp; ++t) {
            const double v = value(t, c);
            s += v;
            q += v * v;
        }
        if (acc[c] != s || acc[nchans + c] != q) {
            std::printf("FAILED: packed channel stats nbits %d nchans %zu channel %zu\n", nbits, nchans, c);
            ++fails;
            return;
        }
    }
}

void run_packed_errors()
{
    std::vector<uint8_t> x(64, 0xA5);
    std::vector<float> out(16), m(16);
    std::vector<int64_t> del(16, 0);
    std::vector<double> acc(32, 0.0);
    size_t rb = 0;
    expect(rt_dedisp_row_bytes(RT_DEDISP_U8, 7, &rb) == RT_OK && rb == 7, "row_bytes, uint8");
    expect(rt_dedisp_row_bytes(RT_DEDISP_I8, 7, &rb) == RT_OK && rb == 7, "row_bytes, int8");
    expect(rt_dedisp_row_bytes(RT_DEDISP_F32, 7, &rb) == RT_OK && rb == 28, "row_bytes, float32");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U1, 24, &rb) == RT_OK && rb == 3, "row_bytes, 1 bit");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U16, 3, &rb) == RT_OK && rb == 6, "row_bytes, 16 bit");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U1, 12, &rb) == RT_EINVAL, "row_bytes: 12 one-bit channels");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U2, 6, &rb) == RT_EINVAL, "row_bytes: 6 two-bit channels");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U4, 3, &rb) == RT_EINVAL, "row_bytes: 3 four-bit channels");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U4, 0, &rb) == RT_EINVAL, "row_bytes: nchans == 0");
    expect(rt_dedisp_row_bytes(0x108, 8, &rb) == RT_EINVAL, "row_bytes: unknown code");
    expect(rt_dedisp_row_bytes(RT_DEDISP_U4, 2, nullptr) == RT_EINVAL, "row_bytes: bytes is NULL");
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U1, 4, 12, del.data(), nullptr, 1, 0, 4, out.data()) == RT_EINVAL,
           "host: rows are not whole bytes");
    expect(rt_zero_dm_mean_host(x.data(), RT_DEDISP_U2, 4, 6, nullptr, m.data()) == RT_EINVAL,
           "mean: rows are not whole bytes");
    expect(rt_channel_stats_host(x.data(), RT_DEDISP_U4, 4, 3, acc.data()) == RT_EINVAL,
           "stats: rows are not whole bytes");
    expect(rt_dedisperse_host(x.data(), 0x108, 4, 8, del.data(), nullptr, 1, 0, 4, out.data()) == RT_EINVAL,
           "host: unknown code in the packed range");
}

void run_rfi_errors()
{
    std::vector<uint8_t> x(10 * 2, 1);
    std::vector<float> out(7), m(10);
    std::vector<int64_t> d2{0, 3};
    std::vector<double> acc(4, 0.0);
    expect(rt_dedisperse_host_opt(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 7, out.data(), 2u) ==
               RT_EINVAL, "unknown flag bit");
    expect(rt_dedisperse_host_opt(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 8, out.data(),
                                  RT_DEDISP_ZERO_DM) == RT_EINVAL, "nout + max_delay > nsamp (zero-DM)");
    expect(rt_dedisperse_host_opt(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 7, out.data(),
                                  RT_DEDISP_ZERO_DM) == RT_OK, "zero-DM of a constant block");
    for (float v : out) expect(v == 0.0f, "a constant block is all mean");
    std::vector<uint8_t> every{1, 1};
    expect(rt_dedisperse_host_opt(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), every.data(), 1, 3, 7, out.data(),
                                  RT_DEDISP_ZERO_DM) == RT_OK, "every channel masked");
    for (float v : out) expect(v == 0.0f, "no unmasked channel: zero");
    expect(rt_zero_dm_mean_host(x.data(), RT_DEDISP_U8, 10, 2, every.data(), m.data()) == RT_OK, "mean, all masked");
    for (float v : m) expect(v == 0.0f, "no unmasked channel: m = 0");
    expect(rt_zero_dm_mean_host(x.data(), 7, 10, 2, nullptr, m.data()) == RT_EINVAL, "mean: unknown type code");
    expect(rt_zero_dm_mean_host(x.data(), RT_DEDISP_U8, 10, 0, nullptr, m.data()) == RT_EINVAL, "mean: nchans == 0");
    expect(rt_channel_stats_host(x.data(), 7, 10, 2, acc.data()) == RT_EINVAL, "stats: unknown type code");
    expect(rt_channel_stats_host(x.data(), RT_DEDISP_U8, 10, 0, acc.data()) == RT_EINVAL, "stats: nchans == 0");
    expect(rt_channel_stats_host(x.data(), RT_DEDISP_U8, 10, 2, nullptr) == RT_EINVAL, "stats: acc is NULL");
    expect(rt_channel_stats_host(x.data(), RT_DEDISP_U8, 10, 2, acc.data()) == RT_OK, "stats");
    expect(acc[0] == 10.0 && acc[1] == 10.0 && acc[2] == 10.0 && acc[3] == 10.0, "stats of a block of ones");
}

void run_errors()
{
    std::vector<double> f{400.0, 390.0}, dm{1.0};
    std::vector<int64_t> del(2);
    int64_t md = 0;
    auto delays = [&](size_t nchans, size_t ndm, double tsamp) {
        return rt_dedisperse_delays(f.data(), nchans, dm.data(), ndm, tsamp, 1.0 / 2.41e-4, del.data(), &md);
    };
    expect(delays(0, 1, 1e-3) == RT_EINVAL, "nchans == 0");
    expect(delays(2, 0, 1e-3) == RT_EINVAL, "ndm == 0");
    expect(delays(2, 1, 0.0) == RT_EINVAL, "tsamp == 0");
    expect(delays(2, 1, -1.0) == RT_EINVAL, "tsamp < 0");
    f[1] = 0.0;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "zero frequency");
    f[1] = -5.0;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "negative frequency");
    f[1] = INFINITY;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "infinite frequency");
    f[1] = NAN;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "NaN frequency");
    f[1] = 390.0;
    dm[0] = -1.0;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "negative DM");
    dm[0] = NAN;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "NaN DM");
    dm[0] = INFINITY;
    expect(delays(2, 1, 1e-3) == RT_EINVAL, "infinite DM");
    dm[0] = 1.0;
    expect(delays(2, 1, 1e-16) == RT_EINVAL, "delay of 2^31 or more");
    expect(delays(2, 1, 1e-3) == RT_OK, "valid call after the errors");

    std::vector<uint8_t> x(10 * 2, 1);
    std::vector<float> out(10);
    std::vector<int64_t> d2{0, 3};
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 8, out.data()) == RT_EINVAL,
           "nout + max_delay > nsamp");
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 7, out.data()) == RT_OK,
           "nout + max_delay == nsamp");
    expect(out[6] == 2.0f, "last output reads the last sample");
    expect(rt_dedisperse_host(x.data(), 7, 10, 2, d2.data(), nullptr, 1, 3, 7, out.data()) == RT_EINVAL,
           "unknown type code");
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 2, 7, out.data()) == RT_EINVAL,
           "delay above max_delay");
    d2[1] = -1;
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U8, 10, 2, d2.data(), nullptr, 1, 3, 7, out.data()) == RT_EINVAL,
           "negative delay");
    expect(rt_dedisperse_host(x.data(), RT_DEDISP_U8, 10, 0, d2.data(), nullptr, 1, 3, 7, out.data()) == RT_EINVAL,
           "nchans == 0 (host)");
}

// rt_dedisperse_span_plan against the closed forms riptide_amd.h states: every
// lo % 4, spreads around both thresholds, large delays, and the refusals
void run_span_plan()
{
    const int64_t bases[] = {0, 1, 2, 3, 4, 7, 1000, 1001, 1002, 1003, 2147482000ll};
    for (int64_t lo : bases)
        for (int64_t spread = 0; spread <= 1200; ++spread) {
            const int64_t hi = lo + spread;
            if (hi >= 2147483648ll) break;
            size_t ndw = 0;
            int staged = -1;
            expect(rt_dedisperse_span_plan(1, lo, hi, &ndw, &staged) == RT_OK, "span plan, 8-bit rows");
            const int64_t w8 = hi - (lo & ~(int64_t)3);
            expect((int64_t)ndw == (256 + w8 + 3) / 4 && staged == (w8 <= 800), "span plan table, 8-bit rows");
            ndw = 0;
            staged = -1;
            expect(rt_dedisperse_span_plan(4, lo, hi, &ndw, &staged) == RT_OK, "span plan, float rows");
            expect((int64_t)ndw == 256 + spread && staged == (spread <= 264), "span plan table, float rows");
        }
    size_t ndw = 0;
    int staged = -1;
    expect(rt_dedisperse_span_plan(1, 0, 800, &ndw, &staged) == RT_OK && ndw == 264 && staged == 1,
           "span plan: the last staged 8-bit span is 264 dwords");
    expect(rt_dedisperse_span_plan(1, 3, 800, &ndw, &staged) == RT_OK && ndw == 264 && staged == 1,
           "span plan: lo % 4 == 3 stages a spread of 797");
    expect(rt_dedisperse_span_plan(1, 3, 801, &ndw, &staged) == RT_OK && ndw == 265 && staged == 0,
           "span plan: lo % 4 == 3 reads a spread of 798 directly");
    expect(rt_dedisperse_span_plan(4, 5, 269, &ndw, &staged) == RT_OK && ndw == 520 && staged == 1,
           "span plan: the last staged float span is 520 dwords");
    expect(rt_dedisperse_span_plan(4, 5, 270, &ndw, &staged) == RT_OK && ndw == 521 && staged == 0,
           "span plan: a float spread of 265 is read directly");
    expect(rt_dedisperse_span_plan(1, 0, 0, nullptr, nullptr) == RT_OK, "span plan: null outputs");
    expect(rt_dedisperse_span_plan(1, 0, 2147483647ll, &ndw, &staged) == RT_OK && staged == 0,
           "span plan: the largest delay");
    expect(rt_dedisperse_span_plan(0, 0, 1, &ndw, &staged) == RT_EINVAL, "span plan: esize 0");
    expect(rt_dedisperse_span_plan(2, 0, 1, &ndw, &staged) == RT_EINVAL, "span plan: esize 2");
    expect(rt_dedisperse_span_plan(8, 0, 1, &ndw, &staged) == RT_EINVAL, "span plan: esize 8");
    expect(rt_dedisperse_span_plan(1, 5, 4, &ndw, &staged) == RT_EINVAL, "span plan: lo > hi");
    expect(rt_dedisperse_span_plan(1, -1, 4, &ndw, &staged) == RT_EINVAL, "span plan: negative lo");
    expect(rt_dedisperse_span_plan(4, -3, -2, &ndw, &staged) == RT_EINVAL, "span plan: negative delays");
    expect(rt_dedisperse_span_plan(4, 0, 2147483648ll, &ndw, &staged) == RT_EINVAL, "span plan: hi of 2^31");
}

}  // namespace

int main()
{
    const size_t chans[] = {1, 3, 37, 64, 65};
    for (size_t nchans : chans)
        for (int asc = 0; asc < 2; ++asc)
            for (int dtype = 0; dtype < 3; ++dtype)
                for (int masked = 0; masked < 2; ++masked)
                    for (int single = 0; single < 2; ++single) {
                        if (masked && nchans < 3) continue;
                        run_shape(nchans, asc != 0, dtype, masked != 0, single != 0);
                    }
    for (size_t nchans : chans)
        for (int dtype = 0; dtype < 3; ++dtype)
            for (int masked = 0; masked < 2; ++masked)
                for (int single = 0; single < 2; ++single) {
                    if (masked && nchans < 3) continue;
                    run_rfi_shape(nchans, dtype, masked != 0, single != 0);
                }
    const struct {
        int nbits;
        size_t chans[4];
    } packed[] = {{1, {8, 24, 64, 72}}, {2, {4, 12, 64, 68}}, {4, {2, 6, 64, 66}}, {16, {1, 3, 64, 65}}};
    for (const auto& p : packed)
        for (size_t nchans : p.chans)
            for (int masked = 0; masked < 2; ++masked) run_packed_shape(p.nbits, nchans, masked != 0);
    run_errors();
    run_rfi_errors();
    run_packed_errors();
    run_span_plan();
    if (fails)
        std::printf("dedisp_check: %d failures\n", fails);
    else
        std::printf("dedisp_check OK\n");
    return fails ? 1 : 0;
}
