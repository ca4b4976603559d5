// Host-only checker of the block mask's specification (rt_block_replace_host
// and rt_block_stats_host: dedisp_host.cpp), built with AddressSanitizer +
// UBSan by `make -C riptide_amd/csrc asan`.  Every array is a heap block of
// exactly the size the entry point may touch, so a read past the last sample,
// the last block's cells or the fill, or a write past the last row or the
// last block's statistics, is a sanitizer report.  No device call, and none
// linked.  Usage:
//   blockmask_check
// Runs 1, 8, 24 and 65 channels of every sample type (the packed ones where
// the rows are whole bytes) with block_len in {1, 7, 256, nsamp, nsamp + 9},
// t_origin in {0, 5, block_len - 1} and exactly the blocks the rows need,
// masks none / all / one cell / the last block / one channel / random --
// against a recount by the definitions of riptide_amd.h, in place and out of
// place; the statistics at block_len in {1, 5, 2048, 2049, 5000, > nsamp} on
// 6000 samples against a recount (exact for integers, the stated order for
// float32); then every error return.  Exit status 0 iff all agree.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dedisp_types.hpp"
#include "riptide_amd.h"

namespace {

using rt::dedisp_packed_bits;

uint64_t g_state = 2468;
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

// the bits of sample (t, c) as a 32-bit pattern, by the definitions of riptide_amd.h
uint32_t sample_bits(const unsigned char* x, int dtype, size_t row_bytes, size_t t, size_t c)
{
    const unsigned char* row = x + t * row_bytes;
    if (dtype == RT_DEDISP_U8 || dtype == RT_DEDISP_I8) return row[c];
    if (dtype == RT_DEDISP_F32) {
        uint32_t v;
        std::memcpy(&v, row + 4 * c, 4);
        return v;
    }
    const int nbits = dedisp_packed_bits(dtype);
    if (nbits == 16) return (uint32_t)row[2 * c] | (uint32_t)row[2 * c + 1] << 8;
    const size_t bit = c * (size_t)nbits;
    return (uint32_t)(row[bit >> 3] >> (bit & 7)) & ((1u << nbits) - 1u);
}

// the value of sample (t, c)
double sample_value(const unsigned char* x, int dtype, size_t row_bytes, size_t t, size_t c)
{
    const uint32_t b = sample_bits(x, dtype, row_bytes, t, c);
    if (dtype == RT_DEDISP_I8) return (double)(signed char)b;
    if (dtype == RT_DEDISP_F32) {
        float v;
        std::memcpy(&v, &b, 4);
        return (double)v;
    }
    return (double)b;
}

// the bits a flagged sample of channel c must hold
uint32_t fill_bits(const std::vector<unsigned char>& fill, int dtype, size_t c)
{
    const int nbits = dedisp_packed_bits(dtype);
    if (dtype == RT_DEDISP_F32) {
        uint32_t v;
        std::memcpy(&v, fill.data() + 4 * c, 4);
        return v;
    }
    if (nbits == 16) {
        uint16_t v;
        std::memcpy(&v, fill.data() + 2 * c, 2);
        return v;
    }
    if (nbits) return fill[c] & ((1u << nbits) - 1u);
    return fill[c];
}

std::vector<unsigned char> random_block(int dtype, size_t nsamp, size_t nchans, size_t row_bytes)
{
    std::vector<unsigned char> x(nsamp * row_bytes);
    if (dtype == RT_DEDISP_F32) {
        for (size_t i = 0; i < nsamp * nchans; ++i) {
            const float v = (float)((double)draw() / 4294967296.0 - 0.5) * 100.0f;
            std::memcpy(x.data() + 4 * i, &v, 4);
        }
    } else {
        for (unsigned char& v : x) v = (unsigned char)draw();
    }
    return x;
}

void run_replace(size_t nchans, int dtype)
{
    const int nbits = dedisp_packed_bits(dtype);
    if (nbits && nchans * (size_t)nbits % 8) return;   // rows are not whole bytes: the error cases have it
    const size_t nsamp = 300;
    size_t row_bytes = 0;
    expect(rt_dedisp_row_bytes(dtype, nchans, &row_bytes) == RT_OK, "row_bytes");
    const std::vector<unsigned char> x = random_block(dtype, nsamp, nchans, row_bytes);
    std::vector<unsigned char> fill(nchans * rt::dedisp_fill_bytes(dtype));
    for (unsigned char& v : fill) v = (unsigned char)draw();
    const size_t lens[] = {1, 7, 256, nsamp, nsamp + 9};
    for (size_t block_len : lens) {
        const size_t origins[] = {0, 5, block_len - 1};
        for (size_t t_origin : origins) {
            const size_t nblocks = (t_origin + nsamp + block_len - 1) / block_len;   // exactly what the rows need
            for (int kind = 0; kind < 6; ++kind) {
                std::vector<uint8_t> cells(nblocks * nchans, 0);
                if (kind == 1) cells.assign(cells.size(), 1);
                if (kind == 2) cells[(nblocks / 2) * nchans + nchans / 2] = 1;
                if (kind == 3)
                    for (size_t c = 0; c < nchans; ++c) cells[(nblocks - 1) * nchans + c] = 200;
                if (kind == 4)
                    for (size_t b = 0; b < nblocks; ++b) cells[b * nchans + nchans / 3] = 1;
                if (kind == 5)
                    for (uint8_t& v : cells) v = draw() % 10 < 3;
                const rt_block_mask bm{cells.data(), nblocks, block_len, (uint64_t)t_origin, fill.data()};
                std::vector<unsigned char> out(x.size(), 0xAA);
                expect(rt_block_replace_host(x.data(), dtype, nsamp, nchans, &bm, out.data()) == RT_OK, "replace");
                bool same = true;
                for (size_t t = 0; t < nsamp && same; ++t)
                    for (size_t c = 0; c < nchans; ++c) {
                        const bool flag = cells[(t_origin + t) / block_len * nchans + c] != 0;
                        const uint32_t want = flag ? fill_bits(fill, dtype, c) : sample_bits(x.data(), dtype, row_bytes, t, c);
                        if (sample_bits(out.data(), dtype, row_bytes, t, c) != want) {
                            std::printf("FAILED: nchans %zu dtype %d block_len %zu t_origin %zu kind %d at (%zu, %zu)\n",
                                        nchans, dtype, block_len, t_origin, kind, t, c);
                            ++fails;
                            same = false;
                            break;
                        }
                    }
                if (kind == 0) expect(out == x, "no cell flagged: a copy");
                std::vector<unsigned char> inplace = x;   // out may be x
                expect(rt_block_replace_host(inplace.data(), dtype, nsamp, nchans, &bm, inplace.data()) == RT_OK,
                       "replace in place");
                expect(inplace == out, "in place equals out of place");
            }
        }
    }
    std::vector<unsigned char> out(x.size(), 0xAA);
    expect(rt_block_replace_host(x.data(), dtype, nsamp, nchans, nullptr, out.data()) == RT_OK, "no mask");
    expect(out == x, "no mask: a copy");
}

void run_stats(size_t nchans, int dtype)
{
    const int nbits = dedisp_packed_bits(dtype);
    if (nbits && nchans * (size_t)nbits % 8) return;
    const size_t nsamp = 6000, kChunk = 2048;
    size_t row_bytes = 0;
    expect(rt_dedisp_row_bytes(dtype, nchans, &row_bytes) == RT_OK, "row_bytes");
    const std::vector<unsigned char> x = random_block(dtype, nsamp, nchans, row_bytes);
    const size_t lens[] = {1, 5, 2048, 2049, 5000, nsamp + 1};
    for (size_t block_len : lens) {
        const size_t nblk = (nsamp + block_len - 1) / block_len;
        std::vector<double> stats(nblk * 2 * nchans, -7.0);
        expect(rt_block_stats_host(x.data(), dtype, nsamp, nchans, block_len, stats.data()) == RT_OK, "block_stats");
        for (size_t b = 0; b < nblk; ++b) {
            const size_t start = b * block_len, stop = start + block_len < nsamp ? start + block_len : nsamp;
            for (size_t c = 0; c < nchans; ++c) {
                double s = 0.0, q = 0.0;
                for (size_t t0 = start; t0 < stop; t0 += kChunk) {
                    double ps[4] = {0, 0, 0, 0}, pq[4] = {0, 0, 0, 0};
                    for (size_t t = t0; t < stop && t < t0 + kChunk; ++t) {
                        const double v = sample_value(x.data(), dtype, row_bytes, t, c);
                        ps[(t - t0) & 3] += v;
                        pq[(t - t0) & 3] += v * v;
                    }
                    s += ((ps[0] + ps[1]) + ps[2]) + ps[3];
                    q += ((pq[0] + pq[1]) + pq[2]) + pq[3];
                }
                if (stats[(b * 2) * nchans + c] != s || stats[(b * 2 + 1) * nchans + c] != q) {
                    std::printf("FAILED: stats nchans %zu dtype %d block_len %zu block %zu channel %zu\n", nchans, dtype,
                                block_len, b, c);
                    ++fails;
                    return;
                }
            }
        }
    }
}

void run_errors()
{
    const size_t nsamp = 20, nchans = 8;
    std::vector<uint8_t> x(nsamp * nchans, 1), out(nsamp * nchans), cells(2 * nchans, 1), fill(nchans, 9);
    rt_block_mask bm{cells.data(), 2, 10, 0, fill.data()};
    const auto call = [&](int dtype, size_t ns, size_t nch) {
        return rt_block_replace_host(x.data(), dtype, ns, nch, &bm, out.data());
    };
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_OK, "accepted");
    for (uint8_t v : out) expect(v == 9, "all filled");
    bm.t_origin = 1;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "rows past the mask (t_origin)");
    expect(std::strstr(rt_last_error(), "reach past the mask") != nullptr, "rows past the mask message");
    expect(call(RT_DEDISP_U8, nsamp - 1, nchans) == RT_OK, "one row fewer fits");
    bm.t_origin = 0;
    bm.nblocks = 1;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "rows past the mask (nblocks)");
    expect(call(RT_DEDISP_U8, 10, nchans) == RT_OK, "the rows of one block");
    bm.nblocks = 2;
    bm.t_origin = ~0ull;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "t_origin + nsamp overflows 64 bits");
    // the same t_origin under cells said to cover more than 2^64 samples: the 64-bit sum would wrap
    bm.nblocks = (size_t)1 << 40;
    bm.block_len = (size_t)1 << 40;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "t_origin + nsamp overflows under a mask past 2^64");
    expect(std::strstr(rt_last_error(), "overflows 64 bits") != nullptr, "overflow message");
    bm.t_origin = ~0ull - nsamp + 1;   // t_origin + nsamp == 2^64
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "t_origin + nsamp == 2^64");
    bm.nblocks = 2;
    bm.block_len = 10;
    bm.t_origin = 0;
    bm.block_len = 0;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "block_len == 0");
    bm.block_len = 10;
    bm.cells = nullptr;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "NULL cells");
    bm.cells = cells.data();
    bm.fill = nullptr;
    expect(call(RT_DEDISP_U8, nsamp, nchans) == RT_EINVAL, "NULL fill");
    bm.fill = fill.data();
    expect(call(7, nsamp, nchans) == RT_EINVAL, "unknown type");
    expect(call(RT_DEDISP_U8, nsamp, 0) == RT_EINVAL, "nchans == 0");
    expect(call(RT_DEDISP_U2, nsamp, 3) == RT_EINVAL, "rows that are not whole bytes");
    expect(rt_block_replace_host(nullptr, RT_DEDISP_U8, nsamp, nchans, &bm, out.data()) == RT_EINVAL, "NULL x");
    expect(rt_block_replace_host(x.data(), RT_DEDISP_U8, nsamp, nchans, &bm, nullptr) == RT_EINVAL, "NULL out");
    expect(rt_block_replace_host(nullptr, RT_DEDISP_U8, 0, nchans, &bm, nullptr) == RT_OK, "no rows: nothing to do");

    std::vector<double> stats(2 * 2 * nchans);
    expect(rt_block_stats_host(x.data(), RT_DEDISP_U8, nsamp, nchans, 10, stats.data()) == RT_OK, "stats accepted");
    for (double v : stats) expect(v == 10.0, "sums of ones");
    expect(rt_block_stats_host(x.data(), RT_DEDISP_U8, nsamp, nchans, 0, stats.data()) == RT_EINVAL, "stats block_len == 0");
    expect(rt_block_stats_host(x.data(), 7, nsamp, nchans, 10, stats.data()) == RT_EINVAL, "stats unknown type");
    expect(rt_block_stats_host(x.data(), RT_DEDISP_U8, nsamp, 0, 10, stats.data()) == RT_EINVAL, "stats nchans == 0");
    expect(rt_block_stats_host(x.data(), RT_DEDISP_U4, nsamp, 3, 10, stats.data()) == RT_EINVAL, "stats rows not whole bytes");
    expect(rt_block_stats_host(nullptr, RT_DEDISP_U8, nsamp, nchans, 10, stats.data()) == RT_EINVAL, "stats NULL x");
    expect(rt_block_stats_host(x.data(), RT_DEDISP_U8, nsamp, nchans, 10, nullptr) == RT_EINVAL, "stats NULL stats");
    expect(rt_block_stats_host(nullptr, RT_DEDISP_U8, 0, nchans, 10, nullptr) == RT_OK, "stats of no rows");
}

}  // namespace

int main()
{
    const int dtypes[] = {RT_DEDISP_U8, RT_DEDISP_I8, RT_DEDISP_F32, RT_DEDISP_U1, RT_DEDISP_U2, RT_DEDISP_U4,
                          RT_DEDISP_U16};
    const size_t chans[] = {1, 8, 24, 65};
    for (size_t nchans : chans)
        for (int dtype : dtypes) {
            run_replace(nchans, dtype);
            run_stats(nchans, dtype);
        }
    run_errors();
    if (fails) {
        std::printf("blockmask_check: %d FAILED\n", fails);
        return 1;
    }
    std::printf("blockmask_check OK\n");
    return 0;
}
