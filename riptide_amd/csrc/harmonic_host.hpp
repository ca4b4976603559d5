// Host side of the harmonic flagging (rt_flag_harmonics): the layout of one
// tile of the pair matrix as the device leaves it, and its resolution into
// parent / hnum / hden.  No HIP header.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>

#include "harmonic.hpp"

namespace rt {

// A tile in host memory: a 16-byte header (the near count), the near list of
// kHNearCap (i, j) pairs, then rows x wpr 64-bit words.
constexpr uint32_t kHNearCap = 4096;
constexpr size_t kHHeaderBytes = 16;
struct HNearPair {
    uint32_t x, y;   // i, j: the device's uint2
};
constexpr size_t kHWordsOff = kHHeaderBytes + (size_t)kHNearCap * sizeof(HNearPair);

struct HInputs {
    const double *freq, *snr, *ducy, *dm;
    HCand at(size_t i) const { return HCand{freq[i], snr[i], ducy[i], dm[i]}; }
};

struct HTileCounts {
    uint64_t near_pairs = 0, host_rows = 0;
};

// Resolves rows [i0, i0 + r) of the n ranked clusters.  words: r x wpr, bit j
// of row i = the device's htest(i, j) for j > i; near: the first
// min(count, kHNearCap) pairs the host must decide.  With count above the cap
// the list is incomplete: neither it nor the words are read, and every
// unclaimed row is tested on the host.  Tiles are resolved in rank order.
inline HTileCounts hresolve_tile(uint32_t count, const HNearPair* near, uint64_t* words, size_t i0, size_t r,
                                 size_t wpr, size_t n, const HInputs& in, const HParams& P, int32_t* parent,
                                 int64_t* hnum, int64_t* hden)
{
    HTileCounts tc;
    auto assign = [&](size_t i, size_t j) {
        const HDiag d = hdiag_pair(in.at(i), in.at(j), P);
        parent[j] = (int32_t)i;
        hnum[j] = d.num;
        hden[j] = d.den;
    };
    const bool overflow = count > kHNearCap;
    if (!overflow) {
        // the host's verdict replaces the device's for every near pair
        for (uint32_t k = 0; k < count; ++k) {
            const size_t i = near[k].x, j = near[k].y;
            if (i < i0 || i >= i0 + r || j <= i || j >= n) throw std::runtime_error("harmonics: bad near pair");
            uint64_t& w = words[(i - i0) * wpr + j / 64];
            const uint64_t bit = (uint64_t)1 << (j % 64);
            w = htest_pair(in.at(i), in.at(j), P, nullptr) ? (w | bit) : (w & ~bit);
        }
        tc.near_pairs = count;
    }
    // rank order: a fundamental claims every unclaimed cluster related to it
    for (size_t i = i0; i < i0 + r; ++i) {
        if (parent[i] >= 0) continue;
        if (overflow) {
            tc.host_rows++;
            for (size_t j = i + 1; j < n; ++j)
                if (parent[j] < 0 && htest_pair(in.at(i), in.at(j), P, nullptr)) assign(i, j);
            continue;
        }
        const uint64_t* row = words + (i - i0) * wpr;
        for (size_t w = i / 64; w < wpr; ++w) {
            for (uint64_t bits = row[w]; bits; bits &= bits - 1) {
                const size_t j = w * 64 + (size_t)__builtin_ctzll(bits);
                if (j <= i || j >= n) throw std::runtime_error("harmonics: bit outside the upper triangle");
                if (parent[j] < 0) assign(i, j);
            }
        }
    }
    return tc;
}

}  // namespace rt
