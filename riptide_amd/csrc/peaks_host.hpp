// Peak clustering shared by the host and the device: the tail of riptide's
// find_peaks_single (riptide/peak_detection.py:130-141) for one (trial, width)
// column, the reference's arithmetic operation for operation.  Compiled with
// -ffp-contract=off everywhere, so np.polyval's y * x + c is two roundings on
// both sides.
//
//   selected   s > polyval(coeffs, logf[i]) and s > smin, s = (double)snr[i]
//              (a NaN fails both comparisons; +inf passes like any value)
//   clusters   the selected rows in ascending order, a new one where
//              fabs(freqs[i] - freqs[j]) > r against the previous selected
//              row j (cluster1d: np.abs(np.diff(x)) > r, one rounded
//              subtraction, strict)
//   peak       np.argmax over the cluster as cluster1d returns it, sorted by
//              ascending frequency: of the rows attaining the cluster's
//              maximum, the one of lowest frequency.  On a grid whose
//              frequencies rise with the row that is the first (lowest) row;
//              on a plan's grid (periods rise, frequencies fall:
//              freqs[L - 1] < freqs[0]) it is the last.  peak_last_wins().
//
// find_peaks_column is the specification: a serial walk.  The kernels
// (peaks_kernels.hip find_peaks_chunk_kernel / find_peaks_join_kernel) share
// peak_selected, peak_breaks and peak_better with it.  No HIP header.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>

#include "common.hpp"

namespace rt {

// np.polyval(c, x): y = y * x + c[k], highest degree first
RT_HD inline double peak_threshold(const double* c, uint32_t ncoef, double x)
{
    double y = 0.0;
    for (uint32_t k = 0; k < ncoef; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
        y = __dadd_rn(__dmul_rn(y, x), c[k]);
#else
        y = y * x + c[k];       // -ffp-contract=off: two roundings
#endif
    }
    return y;
}

RT_HD inline bool peak_selected(float snr, double thr, double smin)
{
    const double s = (double)snr;
    return s > thr && s > smin;
}

// a new cluster starts at a selected row of frequency f whose previous
// selected row has frequency fprev
RT_HD inline bool peak_breaks(double f, double fprev, double r) { return fabs(f - fprev) > r; }

// the tie rule of a grid: the later of two equal maxima wins when the
// frequencies fall with the row
RT_HD inline bool peak_last_wins(const double* freqs, size_t L) { return L > 1 && freqs[L - 1] < freqs[0]; }

// whether a later row replaces the cluster's best: strictly greater, or equal
// too when the last maximum wins (selected values are never NaN).  Either
// rule is an associative choice, so a scan applies it as the serial walk does.
RT_HD inline bool peak_better(float later, float best, bool last_wins)
{
    return last_wins ? later >= best : later > best;
}

// One column: snr[i * stride], i < L.  Writes the first `cap` clusters' peaks
// (ascending rows) and returns the number of clusters, which may exceed cap.
inline uint32_t find_peaks_column(const float* snr, size_t stride, size_t L, const double* logf, const double* freqs,
                                  const double* coeffs, uint32_t ncoef, double smin, double r, uint32_t* rows,
                                  float* out, size_t cap)
{
    uint64_t count = 0;
    bool open = false;
    uint32_t best = 0;
    float best_snr = 0.f;
    double fprev = 0.0;
    const bool last_wins = peak_last_wins(freqs, L);
    auto close = [&] {
        if (count < cap) {
            rows[count] = best;
            out[count] = best_snr;
        }
        ++count;
    };
    for (size_t i = 0; i < L; ++i) {
        const float v = snr[i * stride];
        if (!peak_selected(v, peak_threshold(coeffs, ncoef, logf[i]), smin)) continue;
        if (open && peak_breaks(freqs[i], fprev, r)) {
            close();
            open = false;
        }
        if (!open || peak_better(v, best_snr, last_wins)) {
            best = (uint32_t)i;
            best_snr = v;
        }
        open = true;
        fprev = freqs[i];
    }
    if (open) close();
    return count > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)count;
}

// ---- device staging (find_peaks_chunk_kernel -> find_peaks_join_kernel)
constexpr uint32_t kPeakChunkRows = 1024;   // default rows per chunk
constexpr uint32_t kPeakChunkMax = 1u << 20;
constexpr uint32_t kPeakWidthGroup = 32;    // widths one workgroup takes (128 B of a row)

// What a chunk leaves for one width: its clusters' count, its first and last
// selected rows' frequencies (all the join needs), then n records.
struct PeakChunkHead {
    uint32_t n, pad;
    double f_first, f_last;
};
struct PeakRecord {
    uint32_t row;
    float snr;
};

// rows per chunk of a launch: the caller's value rounded up to a multiple of
// 64 (a wave's step), the default for 0
inline uint32_t peak_chunk_rows(size_t chunk_rows)
{
    if (!chunk_rows) return kPeakChunkRows;
    if (chunk_rows > kPeakChunkMax) return kPeakChunkMax;
    return (uint32_t)((chunk_rows + 63) / 64 * 64);
}
inline uint64_t peak_chunks(uint64_t L, uint32_t chunk) { return (L + chunk - 1) / chunk; }
// the workspace: per (trial, width) nchunks heads, then nchunks * chunk
// records (a chunk's worst case: every row a cluster of its own)
inline uint64_t peak_workspace_bytes(uint64_t batch, uint64_t L, uint64_t W, uint32_t chunk)
{
    const uint64_t nch = peak_chunks(L, chunk);
    return batch * W * nch * (sizeof(PeakChunkHead) + (uint64_t)chunk * sizeof(PeakRecord));
}
// the same for a caller's shape, with the launch's limits (std::invalid_argument)
inline size_t checked_peak_workspace(size_t batch, size_t L, size_t W, size_t chunk_rows)
{
    if (L >= (1ull << 32)) throw std::invalid_argument("find_peaks: length must be below 2^32");
    if (batch > 65535 || W > 65535ull * kPeakWidthGroup || (uint64_t)batch * W > 0x7FFFFFFFull)
        throw std::invalid_argument("find_peaks: batch x widths too large");
    if (chunk_rows > kPeakChunkMax) throw std::invalid_argument("find_peaks: chunk_rows above 2^20");
    const uint32_t chunk = peak_chunk_rows(chunk_rows);
    // batch * W < 2^31 columns of less than 2^37 bytes each
    const uint64_t per_column = peak_workspace_bytes(1, L, 1, chunk);
    if (batch && W && per_column > (1ull << 62) / ((uint64_t)batch * W))
        throw std::invalid_argument("find_peaks: workspace size overflows");
    return (size_t)peak_workspace_bytes(batch, L, W, chunk);
}

}  // namespace rt
