// Single-pulse search of normalised series: the host specification of the
// boxcar S/N, the centred best width and the local-maximum rule, and the launch
// plan of the device form.  No HIP header: shared by the kernels
// (pulse_kernels.hip), the C ABI (capi_pulse.cpp, pulse_host.cpp) and the
// sanitizer checker (pulse_check_main.cpp).
//
// Summation order.  A row is cut into segments of kPulseSeg = 1024 samples and
// a segment into 64 runs of kPulseRun = 16 samples (samples past the row's end
// count as 0.0f).  All arithmetic is IEEE double, one rounded operation per
// step, no FMA:
//
//   r[0] = (double)x[0], r[i] = r[i - 1] + (double)x[i]     inside a run, i < 16
//   base[0] = 0.0, base[j + 1] = base[j] + r[15] of run j   the runs of a segment, j < 64
//   I[u] = base[run of u] + r[position of u]                inclusive partial sum at sample u
//   E[u] = 0.0 when u is a segment's first sample, else I[u - 1]
//   tot[g] = I[last sample of segment g]
//
// The partial sums restart at every segment, so a tile needs nothing of the
// row before the segment its halo starts in.  The sum of the window [a, e),
// e = a + w, with a in segment ga and e - 1 in segment ge:
//
//   ga == ge:  d = I[e - 1] - E[a]
//   ga <  ge:  d = (tot[ga] - E[a]), then + tot[g] for g = ga + 1 .. ge - 1 in
//              order, then + I[e - 1]
//
//   s = (float)(d / sqrt((double)w))
//
// On dyadic inputs every step is exact, and s is the float32 of the exact
// window sum over sqrt(w); in general d differs from a difference of
// whole-row prefix sums by rounding (and is the more accurate of the two:
// its terms are sums of at most 1024 samples).
//
// best / kbest: the widths are tried in ascending k from best = -inf,
// kbest = -1; a width whose window [t - w/2, t - w/2 + w) lies inside the row
// replaces the best when s > best (a plain float compare).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <vector>

#include "capi_common.hpp"

namespace rt {

constexpr uint32_t kPulseMaxWidth = RT_PULSE_MAX_WIDTH;   // widths and the radius
constexpr uint32_t kPulseSeg = RT_PULSE_SEGMENT;          // the partial sums restart
constexpr uint32_t kPulseRun = 16;                        // sequential run: one lane's samples
constexpr uint32_t kPulseSegSlots = (kPulseSeg / kPulseRun) * (kPulseRun + 1);   // a segment in LDS: 17 slots per run
constexpr uint32_t kPulseTile = 4096;                     // outputs of one workgroup
constexpr uint32_t kPulseThreads = 1024;
constexpr uint32_t kPulseLdsMax = 160u << 10;             // one workgroup may take a CU's whole LDS
constexpr uint64_t kPulseMaxSamples = RT_PULSE_MAX_SAMPLES;
constexpr uint32_t kPulseMaxSeries = 65535;               // a grid row per series
static_assert(kPulseTile % kPulseSeg == 0 && kPulseSeg == 64 * kPulseRun, "a wave scans a segment");

inline void pulse_check_args(size_t N, size_t ldx, const int32_t* w, size_t K, float threshold, size_t radius)
{
    if (!K) throw std::invalid_argument("single pulse: no trial widths");
    if (!w) throw std::invalid_argument("single pulse: null widths");
    for (size_t k = 0; k < K; ++k) {
        if (w[k] < 1) throw std::invalid_argument("single pulse: widths must be >= 1");
        if (k && w[k] <= w[k - 1]) throw std::invalid_argument("single pulse: widths must be strictly ascending");
        if ((uint32_t)w[k] > kPulseMaxWidth)
            throw std::invalid_argument("single pulse: a width above RT_PULSE_MAX_WIDTH (6144)");
    }
    if ((uint64_t)w[K - 1] > N) throw std::invalid_argument("single pulse: the largest width exceeds the series");
    if (radius > kPulseMaxWidth) throw std::invalid_argument("single pulse: radius above RT_PULSE_MAX_WIDTH (6144)");
    if (!std::isfinite(threshold)) throw std::invalid_argument("single pulse: the threshold must be finite");
    if (ldx < N) throw std::invalid_argument("single pulse: row stride below the series length");
    if (N > kPulseMaxSamples) throw std::invalid_argument("single pulse: more than 2^30 samples");
}

// I[u] of one row (the header's order); I: N doubles
inline void pulse_partial_sums(const float* x, size_t N, double* I)
{
    for (size_t s0 = 0; s0 < N; s0 += kPulseSeg) {
        double base = 0.0;
        for (size_t r0 = s0; r0 < std::min<size_t>(N, s0 + kPulseSeg); r0 += kPulseRun) {
            double r = 0.0;
            for (size_t i = 0; i < kPulseRun; ++i) {
                const double v = r0 + i < N ? (double)x[r0 + i] : 0.0;
                r = i ? r + v : v;
                if (r0 + i < N) I[r0 + i] = base + r;
            }
            base = base + r;
        }
    }
}

inline double pulse_window_sum(const double* I, size_t a, size_t e)
{
    const size_t ga = a / kPulseSeg, ge = (e - 1) / kPulseSeg;
    const double Ea = a % kPulseSeg ? I[a - 1] : 0.0;
    if (ga == ge) return I[e - 1] - Ea;
    double acc = I[(ga + 1) * kPulseSeg - 1] - Ea;
    for (size_t g = ga + 1; g < ge; ++g) acc += I[(g + 1) * kPulseSeg - 1];
    return acc + I[e - 1];
}

// best [N], kbest [N] of one row; I: the row's partial sums; sq[k] = sqrt((double)w[k])
inline void pulse_best_row(const double* I, size_t N, const int32_t* w, const double* sq, size_t K, float* best,
                           int32_t* kbest)
{
    for (size_t t = 0; t < N; ++t) {
        float bv = -std::numeric_limits<float>::infinity();
        int32_t bk = -1;
        for (size_t k = 0; k < K; ++k) {
            const size_t wk = (size_t)w[k], c = wk / 2;
            if (t < c || t - c + wk > N) continue;
            const float s = (float)(pulse_window_sum(I, t - c, t - c + wk) / sq[k]);
            if (s > bv) {
                bv = s;
                bk = (int32_t)k;
            }
        }
        best[t] = bv;
        kbest[t] = bk;
    }
}

inline bool pulse_is_event(const float* best, size_t N, size_t t, float threshold, size_t R)
{
    const float v = best[t];
    if (!(v >= threshold)) return false;
    for (size_t u = t > R ? t - R : 0; u < t; ++u)
        if (!(v > best[u])) return false;
    for (size_t u = t + 1; u < N && u <= t + R; ++u)
        if (!(v >= best[u])) return false;
    return true;
}

// The specification, sequential.  Returns the number of events found; the
// first `capacity` are written.  best / kbest may be null.
static inline uint64_t single_pulse_host(const float* x, size_t B, size_t N, size_t ldx, const int32_t* w, size_t K,
                                         float threshold, size_t radius, rt_pulse_event* events, size_t capacity,
                                         float* best, int32_t* kbest)
{
    pulse_check_args(N, ldx, w, K, threshold, radius);
    if (B && !x) throw std::invalid_argument("single pulse: null data");
    if (capacity && !events) throw std::invalid_argument("single pulse: null events with a capacity");
    std::vector<double> I(N), sq(K);
    std::vector<float> bv(N);
    std::vector<int32_t> bk(N);
    for (size_t k = 0; k < K; ++k) sq[k] = std::sqrt((double)w[k]);
    uint64_t found = 0;
    for (size_t b = 0; b < B; ++b) {
        pulse_partial_sums(x + b * ldx, N, I.data());
        pulse_best_row(I.data(), N, w, sq.data(), K, bv.data(), bk.data());
        if (best) std::copy(bv.begin(), bv.end(), best + b * N);
        if (kbest) std::copy(bk.begin(), bk.end(), kbest + b * N);
        for (size_t t = 0; t < N; ++t) {
            if (!pulse_is_event(bv.data(), N, t, threshold, radius)) continue;
            if (found < capacity) events[found] = rt_pulse_event{(int32_t)b, (int32_t)t, bk[t], bv[t]};
            ++found;
        }
    }
    return found;
}

// ---- the device form's plan

struct PulseWidth {   // one trial width of the device table
    int32_t w, c;     // width, w / 2
    double sq;        // sqrt((double)w)
};

struct PulsePlan {
    uint32_t tiles = 0;        // per row
    uint32_t chunk = 0;        // outputs (with the radius halo) whose partial sums are in LDS at once
    uint32_t chunk_segs = 0;   // segments of a chunk's samples
    uint32_t best_floats = 0;  // kPulseTile + 2 * radius
    uint32_t lds_bytes = 0;
    // workspace: cursor (256 B) | widths | tile counts u32 | tile pool positions u64 | tile offsets u64 | pool
    size_t off_widths = 0, off_cnt = 0, off_pos = 0, off_off = 0, off_pool = 0, ws_bytes = 0;
};

inline uint32_t pulse_chunk_segs(uint32_t chunk, uint32_t wmax)
{
    // samples [u0 - wmax / 2, u0 - wmax / 2 + chunk + wmax - 1), the start moved down to a segment's
    return (chunk + wmax + 2 * kPulseSeg - 3) / kPulseSeg;
}

inline PulsePlan pulse_plan(size_t B, size_t N, size_t K, size_t capacity, uint32_t wmax, uint32_t radius)
{
    PulsePlan P;
    P.tiles = (uint32_t)((N + kPulseTile - 1) / kPulseTile);
    P.best_floats = kPulseTile + 2 * radius;
    const uint32_t fixed = P.best_floats * 4 + kPulseTile * 2 + 64 * 4 + 64;
    uint32_t chunk = (P.best_floats + kPulseSeg - 1) / kPulseSeg * kPulseSeg;
    while (chunk > kPulseSeg && fixed + pulse_chunk_segs(chunk, wmax) * kPulseSegSlots * 8 > kPulseLdsMax)
        chunk -= kPulseSeg;
    P.chunk = chunk;
    P.chunk_segs = pulse_chunk_segs(chunk, wmax);
    P.lds_bytes = fixed + P.chunk_segs * kPulseSegSlots * 8;
    if (P.lds_bytes > kPulseLdsMax) throw std::logic_error("single pulse: the tile does not fit the LDS");
    const size_t ntiles = B * (size_t)P.tiles;
    P.off_widths = 256;
    P.off_cnt = P.off_widths + align_up(K * sizeof(PulseWidth), 256);
    P.off_pos = P.off_cnt + align_up(ntiles * 4, 256);
    P.off_off = P.off_pos + align_up(ntiles * 8, 256);
    P.off_pool = P.off_off + align_up(ntiles * 8, 256);
    P.ws_bytes = P.off_pool + align_up(capacity * sizeof(rt_pulse_event), 256);
    return P;
}

}  // namespace rt
