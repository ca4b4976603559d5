// Host-only checker of the peak-clustering walk (peaks_host.hpp through
// rt_find_peaks_host), built with AddressSanitizer + UBSan by
// `make -C riptide_amd/csrc asan`.  Every array is a heap block of exactly the
// size the entry point may touch, so a read or write past a column, a
// coefficient row or the cap slots is a sanitizer report.  No device call, and
// none linked.  Usage:
//   peaks_check LENGTH WIDTHS NCOEF CAP SEED
// Prints the clusters of every width; exit status 0 iff the call returned
// RT_OK and its counts agree with a recount of the breaks.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "riptide_amd.h"

int main(int argc, char** argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: peaks_check LENGTH WIDTHS NCOEF CAP SEED\n");
        return 2;
    }
    const size_t L = std::strtoull(argv[1], nullptr, 10), W = std::strtoull(argv[2], nullptr, 10);
    const size_t ncoef = std::strtoull(argv[3], nullptr, 10), cap = std::strtoull(argv[4], nullptr, 10);
    uint64_t state = std::strtoull(argv[5], nullptr, 10) * 2 + 1;
    auto uniform = [&] {   // 53-bit LCG draw in [0, 1)
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(state >> 11) / 9007199254740992.0;
    };
    std::vector<float> snrs(L * W);
    std::vector<double> logf(L), freqs(L), coeffs(W * ncoef, 0.0);
    for (size_t i = 0; i < L; ++i) {
        freqs[i] = 1.0 + 0.001 * (double)i;
        logf[i] = std::log(freqs[i]);
    }
    for (float& v : snrs) v = (float)(12.0 * uniform());
    for (size_t i = 0; i < L * W; i += 97) snrs[i] = i % 2 ? NAN : INFINITY;
    for (size_t iw = 0; iw < W; ++iw) coeffs[iw * ncoef + ncoef - 1] = 9.0;
    const double smin = 6.0, radius = 0.0025;
    std::vector<uint32_t> counts(W), rows(W * cap);
    std::vector<float> out(W * cap);
    if (rt_find_peaks_host(snrs.data(), L, W, logf.data(), freqs.data(), coeffs.data(), ncoef, smin, radius,
                           counts.data(), rows.data(), out.data(), cap)) {
        std::printf("find_peaks: %s\n", rt_last_error());
        return 1;
    }
    for (size_t iw = 0; iw < W; ++iw) {
        // recount: a selected row more than `radius` after the previous one
        uint32_t n = 0;
        double fprev = 0.0;
        bool any = false;
        for (size_t i = 0; i < L; ++i) {
            const double s = (double)snrs[i * W + iw];
            if (!(s > 9.0 && s > smin)) continue;
            if (!any || std::fabs(freqs[i] - fprev) > radius) ++n;
            any = true;
            fprev = freqs[i];
        }
        std::printf("%sw%zu=%u", iw ? " " : "clusters ", iw, counts[iw]);
        if (n != counts[iw]) {
            std::printf("\nwidth %zu: recount %u\n", iw, n);
            return 1;
        }
        for (size_t k = 0; k < cap && k < counts[iw]; ++k)
            if (rows[iw * cap + k] >= L || out[iw * cap + k] != snrs[(size_t)rows[iw * cap + k] * W + iw]) {
                std::printf("\nwidth %zu: record %zu is not a row of the column\n", iw, k);
                return 1;
            }
    }
    std::printf("\n");
    return 0;
}
