// Host-only checker of the sub-band dedispersion specification
// (rt_dedisperse_bands_host: dedisp_host.cpp), built with AddressSanitizer +
// UBSan by `make -C riptide_amd/csrc asan`.  Every array is a heap block of
// exactly the size the entry point may touch, so a read past the last sample,
// a delay row, the mask or the band table, or a write past out's last row, is
// a sanitizer report.  No device call, and none linked.  Usage:
//   bands_check
// Runs 1, 16, 17 and 37 channels with a table of an empty band, one-channel
// bands at both ends, the full band, bands ending at nchans and bands that
// overlap, out of order -- every sample type (the packed ones where the rows
// are whole bytes), with and without a mask and RT_DEDISP_ZERO_DM, nout =
// nsamp - max_delay and nout = 1 -- against a recount and against
// rt_dedisperse_host_opt with a per-band mask; then every error return.  Exit
// status 0 iff all agree.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dedisp_types.hpp"
#include "riptide_amd.h"

namespace {

using rt::dedisp_packed_bits;

uint64_t g_state = 4321;
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

// the value of sample (t, c), by the definitions of riptide_amd.h
double value(const std::vector<unsigned char>& x, int dtype, size_t row_bytes, size_t t, size_t c)
{
    const unsigned char* row = x.data() + t * row_bytes;
    if (dtype == RT_DEDISP_U8) return (double)row[c];
    if (dtype == RT_DEDISP_I8) return (double)(signed char)row[c];
    if (dtype == RT_DEDISP_F32) {
        float v;
        std::memcpy(&v, row + 4 * c, 4);
        return (double)v;
    }
    const int nbits = dedisp_packed_bits(dtype);
    if (nbits == 16) return (double)((unsigned)row[2 * c] | (unsigned)row[2 * c + 1] << 8);
    const size_t bit = c * (size_t)nbits;
    return (double)((row[bit >> 3] >> (bit & 7)) & ((1u << nbits) - 1u));
}

std::vector<uint32_t> band_table(size_t nchans)
{
    const uint32_t n = (uint32_t)nchans;
    std::vector<uint32_t> b = {n / 2, n / 2,   // empty
                               0, 1,           // one channel, the first
                               n - 1, n,       // one channel, the last
                               0, n,           // the full band
                               n / 3, n,       // ends at nchans
                               0, n / 2 + 1,   // overlaps the one before
                               n, n};          // empty, at the end
    return b;
}

void run_shape(size_t nchans, int dtype, bool masked, bool zero_dm, bool single_out)
{
    const int nbits = dedisp_packed_bits(dtype);
    if (nbits && nchans * (size_t)nbits % 8) return;   // rows are not whole bytes: the error cases have it
    const double tsamp = 1e-3, kdm = 1.0 / 2.41e-4;
    const double dms_[] = {0.0, 50.0, 12.5};
    const size_t ndm = 3;
    std::vector<double> freqs(nchans), dms(dms_, dms_ + ndm);
    for (size_t c = 0; c < nchans; ++c) freqs[c] = 400.0 - 32.0 / (double)nchans * (double)c;
    std::vector<int64_t> delays(ndm * nchans);
    int64_t max_delay = -1;
    expect(rt_dedisperse_delays(freqs.data(), nchans, dms.data(), ndm, tsamp, kdm, delays.data(), &max_delay) == RT_OK,
           "delays");
    const size_t nsamp = (size_t)max_delay + 40;
    const size_t nout = single_out ? 1 : nsamp - (size_t)max_delay;
    size_t row_bytes = 0;
    expect(rt_dedisp_row_bytes(dtype, nchans, &row_bytes) == RT_OK, "row_bytes");
    std::vector<unsigned char> x(nsamp * row_bytes);
    if (dtype == RT_DEDISP_F32) {
        for (size_t i = 0; i < nsamp * nchans; ++i) {
            const float v = (float)((double)draw() / 4294967296.0 - 0.5);
            std::memcpy(x.data() + 4 * i, &v, 4);
        }
    } else {
        for (unsigned char& v : x) v = (unsigned char)draw();
    }
    std::vector<uint8_t> mask;
    if (masked) {
        mask.assign(nchans, 0);
        mask[0] = 1;
        if (nchans > 4) mask[nchans / 2] = 1;
    }
    const uint8_t* pm = masked ? mask.data() : nullptr;
    const uint32_t flags = zero_dm ? RT_DEDISP_ZERO_DM : 0u;
    const std::vector<uint32_t> bands = band_table(nchans);
    const size_t nbands = bands.size() / 2;
    std::vector<float> out(ndm * nbands * nout, -1.0f);
    expect(rt_dedisperse_bands_host(x.data(), dtype, nsamp, nchans, delays.data(), pm, ndm, bands.data(), nbands,
                                    max_delay, nout, out.data(), flags) == RT_OK,
           "dedisperse_bands_host");
    const bool exact = !zero_dm && dtype != RT_DEDISP_F32 && dtype != RT_DEDISP_U16;
    std::vector<float> m(nsamp, 0.0f);
    if (zero_dm) expect(rt_zero_dm_mean_host(x.data(), dtype, nsamp, nchans, pm, m.data()) == RT_OK, "zero_dm_mean");
    std::vector<float> plain(ndm * nout);
    std::vector<uint8_t> bmask(nchans);
    for (size_t b = 0; b < nbands; ++b) {
        const size_t lo = bands[2 * b], hi = bands[2 * b + 1];
        // a recount in float64
        for (size_t d = 0; d < ndm; ++d)
            for (size_t t = 0; t < nout; ++t) {
                double ref = 0.0, mag = 0.0;
                for (size_t c = lo; c < hi; ++c) {
                    if (masked && mask[c]) continue;
                    const size_t tt = t + (size_t)delays[d * nchans + c];
                    const float y = (float)value(x, dtype, row_bytes, tt, c) - m[tt];   // as riptide_amd.h defines y
                    const double v = (double)y;
                    ref += v;
                    mag += std::fabs(v);
                }
                const double tol = exact ? 0.0 : (double)(hi - lo) * std::ldexp(1.0, -24) * mag;
                const double got = (double)out[(d * nbands + b) * nout + t];
                if (!(std::fabs(got - ref) <= tol)) {
                    std::printf("FAILED: nchans %zu dtype %d band %zu dm %zu t %zu: %g vs %g\n", nchans, dtype, b, d, t,
                                got, ref);
                    ++fails;
                    return;
                }
            }
        // without the filter, the plain specification with everything outside
        // the band masked is the same sum in the same order: the same bits
        if (zero_dm) continue;
        for (size_t c = 0; c < nchans; ++c) bmask[c] = (uint8_t)(c < lo || c >= hi || (masked && mask[c]));
        expect(rt_dedisperse_host_opt(x.data(), dtype, nsamp, nchans, delays.data(), bmask.data(), ndm, max_delay, nout,
                                      plain.data(), 0u) == RT_OK,
               "dedisperse_host_opt");
        for (size_t d = 0; d < ndm; ++d)
            if (nout && std::memcmp(&out[(d * nbands + b) * nout], &plain[d * nout], nout * 4) != 0) {
                std::printf("FAILED: nchans %zu dtype %d band %zu dm %zu differs from the masked plain call\n", nchans,
                            dtype, b, d);
                ++fails;
                return;
            }
    }
}

void run_errors()
{
    const size_t nsamp = 20, nchans = 8, ndm = 2;
    std::vector<uint8_t> x(nsamp * nchans, 1);
    std::vector<int64_t> delays(ndm * nchans, 3);
    std::vector<float> out(ndm * 2 * 10);
    std::vector<uint32_t> ok = {0, 4, 4, 8};
    const auto call = [&](const uint32_t* b, size_t nb, int dtype, size_t nch, int64_t md, size_t nout, uint32_t fl) {
        return rt_dedisperse_bands_host(x.data(), dtype, nsamp, nch, delays.data(), nullptr, ndm, b, nb, md, nout,
                                        out.data(), fl);
    };
    expect(call(ok.data(), 2, RT_DEDISP_U8, nchans, 3, 10, 0) == RT_OK, "accepted");
    for (size_t i = 0; i < out.size(); ++i) expect(out[i] == 4.0f, "sums of ones");
    expect(call(ok.data(), 0, RT_DEDISP_U8, nchans, 3, 10, 0) == RT_OK, "no band: nothing to do");
    std::vector<uint32_t> inverted = {0, 4, 5, 4}, past = {0, 4, 4, 9};
    expect(call(inverted.data(), 2, RT_DEDISP_U8, nchans, 3, 10, 0) == RT_EINVAL, "lo > hi");
    expect(std::strstr(rt_last_error(), "band 1 [5, 4)") != nullptr, "lo > hi message");
    expect(call(past.data(), 2, RT_DEDISP_U8, nchans, 3, 10, 0) == RT_EINVAL, "hi > nchans");
    expect(std::strstr(rt_last_error(), "band 1 [4, 9)") != nullptr, "hi > nchans message");
    expect(call(nullptr, 2, RT_DEDISP_U8, nchans, 3, 10, 0) == RT_EINVAL, "NULL bands");
    expect(call(ok.data(), 2, 7, nchans, 3, 10, 0) == RT_EINVAL, "unknown type");
    expect(call(ok.data(), 2, RT_DEDISP_U8, nchans, 3, 18, 0) == RT_EINVAL, "nout + max_delay > nsamp");
    expect(call(ok.data(), 2, RT_DEDISP_U8, nchans, 2, 10, 0) == RT_EINVAL, "a delay above max_delay");
    expect(call(ok.data(), 2, RT_DEDISP_U8, nchans, 3, 10, 2) == RT_EINVAL, "unknown flag");
    expect(call(ok.data(), 2, RT_DEDISP_U8, 0, 3, 10, 0) == RT_EINVAL, "nchans == 0");
    std::vector<uint32_t> three = {0, 3};
    expect(call(three.data(), 1, RT_DEDISP_U2, 3, 3, 10, 0) == RT_EINVAL, "rows that are not whole bytes");
}

}  // namespace

int main()
{
    const int dtypes[] = {RT_DEDISP_U8, RT_DEDISP_I8, RT_DEDISP_F32, RT_DEDISP_U1, RT_DEDISP_U2, RT_DEDISP_U4,
                          RT_DEDISP_U16};
    const size_t chans[] = {1, 16, 17, 37};
    for (size_t nchans : chans)
        for (int dtype : dtypes)
            for (int masked = 0; masked < 2; ++masked)
                for (int zero_dm = 0; zero_dm < 2; ++zero_dm) {
                    run_shape(nchans, dtype, masked != 0, zero_dm != 0, false);
                    run_shape(nchans, dtype, masked != 0, zero_dm != 0, true);
                }
    run_errors();
    if (fails) {
        std::printf("bands_check: %d FAILED\n", fails);
        return 1;
    }
    std::printf("bands_check OK\n");
    return 0;
}
