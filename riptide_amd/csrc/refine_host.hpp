// Candidate refinement in period and DM from the sub-band folds: the shift
// tables (the physics, in double), the host specification of the shift-and-add
// search and the launch plan of the device form.  No HIP header: shared by the
// kernels' declarations (kernels.hpp), the C ABI (capi_refine.cpp,
// host_api.cpp) and the sanitizer checker (refine_check_main.cpp).
//
// One candidate is a cube x[b][s][n] (B bands, S sub-integrations, N bins),
// shift tables dshift[k][b] and pshift[j][s] with entries in [0, N), W boxcar
// widths in [1, N - 1] and stdnoise > 0:
//
//   y[k][s][n]    = sum over b = 0..B-1 of x[b][s][(n + dshift[k][b]) mod N]
//   prof[k][j][n] = sum over s = 0..S-1 of y[k][s][(n + pshift[j][s]) mod N]
//   snr[k][j][w]  = snr1 (snr.hpp:37-55) of prof[k][j][:] at width w
//
// Both sums are float32, start from 0.0f and add in index order, one rounded
// addition per term (no FMA, no tree): the device result has the same bits.
//
// Shift tables (refine_shifts), every operation an IEEE double operation in
// this order, left to right where no bracket says otherwise:
//
//   a  = 1.0 / P - 1.0 / P_j
//   c  = ((double)s + 0.5) / (double)S - 0.5
//   vp = floor((double)N * T * a * c + 0.5)            i.e. (((N * T) * a) * c) + 0.5
//   g  = 1.0 / (f[b] * f[b]) - 1.0 / (fmax * fmax)
//   vd = floor((double)N * kdm * (DM_k - DM) * g / P + 0.5)
//                                                       i.e. ((((N * kdm) * (DM_k - DM)) * g) / P) + 0.5
//   shift = fmod(v, N), plus N when that is negative    (exact: v is an integer below 2^31 in magnitude)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "capi_common.hpp"

namespace rt {

constexpr uint32_t kRefineMaxBins = 1024;        // a profile and its prefix sums live in LDS
constexpr uint32_t kRefineThreads = 256;
constexpr uint32_t kRefineStageBytes = 64 << 10; // largest slice (rows x bins floats) a block stages in LDS
// LDS of a block besides the staged slice: 4 wave totals (double), the profile,
// its prefix sums, two buffers of 256 reduced shifts
constexpr uint32_t kRefineFixedLds = 4 * 8 + 2 * kRefineMaxBins * 4 + 2 * kRefineThreads * 4;

inline bool refine_finite_pos(double v) { return std::isfinite(v) && v > 0.0; }

inline int32_t refine_reduce(double v, size_t N, const char* what)
{
    if (!(std::fabs(v) < 2147483648.0)) throw std::invalid_argument(what);
    double r = std::fmod(v, (double)N);
    if (r < 0.0) r += (double)N;
    return (int32_t)r;
}

inline void refine_shifts(double P, double T, size_t N, size_t S, const double* f, size_t B, double dm, double kdm,
                          const double* periods, size_t J, const double* dms, size_t K, int32_t* pshift,
                          int32_t* dshift)
{
    if (!refine_finite_pos(P)) throw std::invalid_argument("refine: the fold period must be positive and finite");
    if (!refine_finite_pos(T)) throw std::invalid_argument("refine: the fold span must be positive and finite");
    if (N < 2) throw std::invalid_argument("refine: bins must be >= 2");
    if (N > 0x7FFFFFFFull) throw std::invalid_argument("refine: too many bins");
    if (!S || !B || !J || !K) throw std::invalid_argument("refine: subints, bands and both trial counts must be >= 1");
    if (!f || !periods || !dms || !pshift || !dshift) throw std::invalid_argument("refine: null argument");
    double fmax = 0.0;
    for (size_t b = 0; b < B; ++b) {
        if (!refine_finite_pos(f[b]))
            throw std::invalid_argument("refine: band frequencies must be positive and finite");
        fmax = std::max(fmax, f[b]);
    }
    for (size_t j = 0; j < J; ++j) {
        if (!refine_finite_pos(periods[j]))
            throw std::invalid_argument("refine: trial periods must be positive and finite");
        const double a = 1.0 / P - 1.0 / periods[j];
        for (size_t s = 0; s < S; ++s) {
            const double c = ((double)s + 0.5) / (double)S - 0.5;
            const double v = std::floor((double)N * T * a * c + 0.5);
            pshift[j * S + s] = refine_reduce(v, N, "refine: a period shift of 2^31 bins or more");
        }
    }
    for (size_t k = 0; k < K; ++k)
        for (size_t b = 0; b < B; ++b) {
            const double g = 1.0 / (f[b] * f[b]) - 1.0 / (fmax * fmax);
            const double v = std::floor((double)N * kdm * (dms[k] - dm) * g / P + 0.5);
            dshift[k * B + b] = refine_reduce(v, N, "refine: a DM shift of 2^31 bins or more");
        }
}

// what both host-buffer forms check of one candidate's tables
inline void refine_check_tables(size_t B, size_t S, size_t N, const int32_t* dshift, size_t K, const int32_t* pshift,
                                size_t J, const uint32_t* widths, size_t W, float stdnoise)
{
    if (N < 2) throw std::invalid_argument("refine: bins must be >= 2");
    if (!S || !B || !J || !K) throw std::invalid_argument("refine: subints, bands and both trial counts must be >= 1");
    if (!W) throw std::invalid_argument("refine: no trial widths");
    if (!(stdnoise > 0)) throw std::invalid_argument("stdnoise must be > 0");
    for (size_t i = 0; i < W; ++i)
        if (!(widths[i] > 0 && widths[i] < N)) throw std::invalid_argument("trial widths must be all > 0 and < columns");
    for (size_t i = 0; i < K * B; ++i)
        if (dshift[i] < 0 || (uint64_t)dshift[i] >= N) throw std::invalid_argument("refine: a DM shift outside [0, bins)");
    for (size_t i = 0; i < J * S; ++i)
        if (pshift[i] < 0 || (uint64_t)pshift[i] >= N)
            throw std::invalid_argument("refine: a period shift outside [0, bins)");
}

// snr1 of one profile (snr.hpp:37-55, kernels.hpp:50-101): sequential prefix
// sums with a double accumulator rounded to float32 as they are stored, the
// wrapped part cps[N + i] = cps[i] + sum in float32.  cps: N + max width floats.
inline void refine_snr1(const float* prof, size_t N, const uint32_t* widths, size_t W, float stdnoise, float* cps,
                        float* out)
{
    const size_t wmax = *std::max_element(widths, widths + W);
    double acc = 0.0;
    for (size_t i = 0; i < N; ++i) {
        acc += (double)prof[i];
        cps[i] = (float)acc;
    }
    const float sum = (float)acc;
    for (size_t i = 0; i < wmax; ++i) cps[N + i] = cps[i] + sum;
    for (size_t iw = 0; iw < W; ++iw) {
        const size_t w = widths[iw];
        const float h = std::sqrt((float)(N - w) / (float)(N * w));
        const float b = (float)w / (float)(N - w) * h;
        float dmax = cps[w] - cps[0];
        for (size_t i = 1; i < N; ++i) {
            const float d = cps[i + w] - cps[i];
            if (d > dmax) dmax = d;
        }
        out[iw] = ((h + b) * dmax - b * sum) / stdnoise;
    }
}

// The specification, sequential: snr [K][J][W], prof [K][J][N] or null.
inline void refine_host(const float* x, size_t B, size_t S, size_t N, const int32_t* dshift, size_t K,
                        const int32_t* pshift, size_t J, const uint32_t* widths, size_t W, float stdnoise, float* snr,
                        float* prof)
{
    if (!x || !dshift || !pshift || !widths || !snr) throw std::invalid_argument("refine: null argument");
    refine_check_tables(B, S, N, dshift, K, pshift, J, widths, W, stdnoise);
    std::vector<float> y(S * N), p(N), cps(2 * N);
    for (size_t k = 0; k < K; ++k) {
        for (size_t s = 0; s < S; ++s)
            for (size_t n = 0; n < N; ++n) {
                float acc = 0.0f;
                for (size_t b = 0; b < B; ++b) acc += x[(b * S + s) * N + (n + (size_t)dshift[k * B + b]) % N];
                y[s * N + n] = acc;
            }
        for (size_t j = 0; j < J; ++j) {
            for (size_t n = 0; n < N; ++n) {
                float acc = 0.0f;
                for (size_t s = 0; s < S; ++s) acc += y[s * N + (n + (size_t)pshift[j * S + s]) % N];
                p[n] = acc;
            }
            refine_snr1(p.data(), N, widths, W, stdnoise, cps.data(), snr + (k * J + j) * W);
            if (prof) std::copy(p.begin(), p.end(), prof + (k * J + j) * N);
        }
    }
}

// ---- the device form's plan

// One candidate of a batched call.  Stage A runs a block per sub-integration,
// stage B a block per DM trial; first_a / first_b are the candidate's first
// block of each launch.
struct RefineCand {
    uint64_t cube_off;    // floats into d_cubes
    uint64_t y_off;       // floats into the workspace's y [ndm][subints][bins]
    uint64_t dshift_off;  // int32 entries into d_shifts: [ndm][bands]
    uint64_t pshift_off;  // [nper][subints]
    uint64_t width_off;   // uint32 entries into d_widths
    uint64_t snr_off;     // floats into d_snr: [ndm][nper][nw]
    uint64_t prof_off;    // floats into d_profiles: [ndm][nper][bins]
    uint32_t bands, subints, bins, ndm, nper, nw;
    float stdnoise;
    uint32_t first_a, first_b;
    uint32_t staged_a, staged_b;   // the block's slice (bands x bins, subints x bins) fits the LDS stage
    uint32_t pad;
};

struct RefinePlan {
    std::vector<RefineCand> cands;
    uint32_t blocks_a = 0, blocks_b = 0;
    uint32_t lds_a = kRefineFixedLds, lds_b = kRefineFixedLds;   // dynamic LDS bytes of each launch
    size_t table_bytes = 0, ws_bytes = 0;
};

// (static: a signature naming the C ABI's struct stays out of the library's
// dynamic symbols)
static inline RefinePlan refine_plan(const rt_refine_spec* specs, size_t nspecs)
{
    RefinePlan P;
    if (!nspecs) return P;
    if (!specs) throw std::invalid_argument("refine: null specs");
    uint64_t na = 0, nb = 0, y_floats = 0;
    P.cands.reserve(nspecs);
    for (size_t i = 0; i < nspecs; ++i) {
        const rt_refine_spec& sp = specs[i];
        if (sp.bins < 2 || sp.bins > kRefineMaxBins) throw std::invalid_argument("refine: bins must be in [2, 1024]");
        if (!sp.bands || !sp.subints || !sp.ndm || !sp.nper)
            throw std::invalid_argument("refine: subints, bands and both trial counts must be >= 1");
        if (!sp.nw) throw std::invalid_argument("refine: no trial widths");
        if (!(sp.stdnoise > 0)) throw std::invalid_argument("stdnoise must be > 0");
        RefineCand c{};
        c.cube_off = sp.cube_off;
        c.dshift_off = sp.dshift_off;
        c.pshift_off = sp.pshift_off;
        c.width_off = sp.width_off;
        c.snr_off = sp.snr_off;
        c.prof_off = sp.prof_off;
        c.bands = sp.bands;
        c.subints = sp.subints;
        c.bins = sp.bins;
        c.ndm = sp.ndm;
        c.nper = sp.nper;
        c.nw = sp.nw;
        c.stdnoise = sp.stdnoise;
        c.y_off = y_floats;
        c.first_a = (uint32_t)na;
        c.first_b = (uint32_t)nb;
        const uint64_t slice_a = (uint64_t)sp.bands * sp.bins * 4, slice_b = (uint64_t)sp.subints * sp.bins * 4;
        c.staged_a = slice_a <= kRefineStageBytes;
        c.staged_b = slice_b <= kRefineStageBytes;
        if (c.staged_a) P.lds_a = std::max<uint32_t>(P.lds_a, kRefineFixedLds + (uint32_t)slice_a);
        if (c.staged_b) P.lds_b = std::max<uint32_t>(P.lds_b, kRefineFixedLds + (uint32_t)slice_b);
        na += sp.subints;
        nb += sp.ndm;
        y_floats += (uint64_t)sp.ndm * sp.subints * sp.bins;
        if (na > 0x7FFFFFFFull || nb > 0x7FFFFFFFull || y_floats > (1ull << 60))
            throw std::invalid_argument("refine: too much work for one call");
        P.cands.push_back(c);
    }
    P.blocks_a = (uint32_t)na;
    P.blocks_b = (uint32_t)nb;
    P.table_bytes = align_up(nspecs * sizeof(RefineCand), 256);
    P.ws_bytes = P.table_bytes + y_floats * sizeof(float);
    return P;
}

}  // namespace rt
