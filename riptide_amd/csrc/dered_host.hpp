// Host geometry of dereddening + normalisation: the scrunch factor and the
// running-median width of a call, the layout of its device workspace
// [lores | rmed | slopes | partials], and the predicates by which the
// launchers (aux_kernels.hip) choose a kernel form for each stage, with
// dered_forms(), which reports those choices for a call (rt_deredden_forms).
// No HIP header.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>

#include "capi_common.hpp"

namespace rt {

// blocks of the fused dereddening + normalisation kernel: 4096 samples each
inline uint64_t dered_norm_blocks(uint64_t n) { return (n + 4095) / 4096; }

struct DeredGeom {
    size_t sf = 1, n_lo = 0, rmed_w = 0;
    size_t lores_floats = 0, rmed_floats = 0, partial_doubles = 0;
    size_t slope_doubles = 0;   // np.interp segment slopes (sf > 1)
};
constexpr uint32_t kNormBlocks = 512;

inline DeredGeom dered_geom(size_t size, size_t ws, size_t minpts, size_t batch, bool deredden)
{
    DeredGeom g;
    if (deredden) {
        if (!(minpts % 2)) throw std::invalid_argument("min_points must be an odd number");
        const double q = (double)ws / (double)minpts;
        g.sf = (size_t)std::max(1.0, q);
        if (g.sf == 1) {
            g.n_lo = size;
            g.rmed_w = ws;
        } else {
            g.n_lo = size / g.sf;
            g.rmed_w = minpts;
            g.lores_floats = align_up(g.n_lo * batch, 64);
            g.slope_doubles = align_up(g.n_lo * batch, 32);
        }
        if (!(g.rmed_w % 2)) throw std::invalid_argument("width must be an odd number");
        if (!(g.rmed_w < g.n_lo)) throw std::invalid_argument("width must be < size");
        g.rmed_floats = align_up(g.n_lo * batch, 64);
    }
    // the unfused normalisation's partials, or the fused one's (two per
    // dereddening block: launch_deredden_normalise), then 2 * batch stats
    g.partial_doubles = std::max<size_t>((size_t)kNormBlocks, deredden ? 2 * dered_norm_blocks(size) : 0) * batch +
                        2 * batch + 8;
    return g;
}

// the 256 bytes: the doubles start at the next 256-byte address after rmed
inline size_t dered_ws_bytes(const DeredGeom& g)
{
    return (g.lores_floats + g.rmed_floats) * 4 + (g.slope_doubles + g.partial_doubles) * 8 + 256;
}

struct DeredWs {
    float* lores;       // lores_floats
    float* rmed;        // rmed_floats
    double* slopes;     // slope_doubles
    double* partials;   // partial_doubles
};

inline DeredWs dered_ws_layout(void* ws, const DeredGeom& g)
{
    DeredWs w;
    w.lores = (float*)ws;
    w.rmed = w.lores + g.lores_floats;
    w.slopes = (double*)align_up((size_t)(w.rmed + g.rmed_floats), 256);
    w.partials = w.slopes + g.slope_doubles;
    return w;
}

// ---- which kernel form a stage takes (the launchers call these; the
// environment switches stay where the launchers read them)
inline bool aligned16(uintptr_t p) { return p % 16 == 0; }

// numpy's pairwise halving of n > 128 addends has one level: both halves are leaves
inline bool np_pairwise_split2(int n)
{
    int n2 = n / 2;
    n2 -= n2 % 8;
    return n <= 128 || n - n2 <= 128;
}

// numpy hands an add-reduction to its pairwise loop in runs of the ufunc
// buffer size (np.getbufsize() elements) and adds the runs' sums in turn
constexpr uint32_t kNpBufSize = 8192;
inline uint32_t scrunch_chunks(uint32_t factor) { return (factor + kNpBufSize - 1) / kNpBufSize; }

// scrunch2_kernel (64 outputs x factor samples staged in LDS) or scrunch_kernel
constexpr uint32_t kScrunchMaxFactor = 256;
inline bool scrunch_staged(uint32_t factor)
{
    return factor <= kScrunchMaxFactor && np_pairwise_split2((int)factor);
}
// scrunch2_kernel stages with 16-byte loads: every block's first sample aligned
inline bool scrunch_vec(uintptr_t x, uint64_t x_stride, uint32_t factor)
{
    return aligned16(x) && x_stride % 4 == 0 && (64 * factor) % 4 == 0;
}

// rmed_run_kernel (LDS span) up to this width, rmed_large_kernel above
constexpr int kRmedSmallMax = 255;
inline bool rmed_small(uint32_t width) { return width <= (uint32_t)kRmedSmallMax; }

// the subtraction reads interp_slope_kernel's table (32-bit sample indices)
inline bool dered_use_slopes(bool have_slopes, uint64_t n, uint64_t n_lo, uint32_t factor)
{
    return have_slopes && factor > 1 && n_lo > 1 && n < (1ull << 31);
}
// deredden_slope_kernel's 16-byte loads and stores
inline bool dered_slope_vec(uintptr_t x, uintptr_t out, uint64_t n, uint64_t x_stride, uint64_t out_stride)
{
    return aligned16(x) && aligned16(out) && x_stride % 4 == 0 && out_stride % 4 == 0 && n < (1ull << 30);
}
// the geometric part of dered_norm_fusable (kernels.hpp)
inline bool dered_norm_fusable_geom(uintptr_t x, uintptr_t out, uint64_t n, uint64_t n_lo, uint32_t factor,
                                    uint64_t x_stride, uint64_t out_stride)
{
    return factor > 1 && n_lo > 1 && dered_slope_vec(x, out, n, x_stride, out_stride);
}
// norm_partial4_kernel / norm_apply4_kernel
inline bool norm_vec_in(uintptr_t x, uint64_t x_stride) { return aligned16(x) && x_stride % 4 == 0; }
inline bool norm_vec_apply(uintptr_t x, uintptr_t out, uint64_t x_stride, uint64_t out_stride)
{
    return norm_vec_in(x, x_stride) && aligned16(out) && out_stride % 4 == 0;
}
// samples one pass of the partial-sum grids covers: kNormBlocks blocks of 256
// threads, one sample (norm_partial_kernel) or two 16-byte loads
// (norm_partial4_kernel's paired loop runs when n / 4 exceeds the grid) each
constexpr uint64_t kNormGridThreads = (uint64_t)kNormBlocks * 256;

// The forms run_deredden_normalise (capi_series.cpp) takes for a call with no
// environment switch set: the RT_* values of rt_dered_forms (riptide_amd.h).
struct DeredForms {
    uint32_t scrunch = 0, scrunch_chunks = 0, rmed = 0, subtract = 0, fused = 0;
    uint32_t norm_partial = 0, norm_passes = 0, norm_apply = 0;
};

inline DeredForms dered_forms(const DeredGeom& g, size_t size, bool deredden, bool normalise, uintptr_t in,
                              uintptr_t out, size_t in_stride, size_t out_stride)
{
    DeredForms f;
    uintptr_t cur = in;
    size_t cur_stride = in_stride;
    if (deredden) {
        if (g.sf > 1) {
            f.scrunch = !scrunch_staged((uint32_t)g.sf) ? RT_SCRUNCH_GENERAL
                        : scrunch_vec(in, in_stride, (uint32_t)g.sf) ? RT_SCRUNCH_STAGED_VEC
                                                                     : RT_SCRUNCH_STAGED;
            f.scrunch_chunks = scrunch_chunks((uint32_t)g.sf);
        }
        f.rmed = rmed_small((uint32_t)g.rmed_w) ? RT_RMED_SMALL : RT_RMED_LARGE;
        f.fused = normalise && g.sf > 1 &&
                  dered_norm_fusable_geom(in, out, size, g.n_lo, (uint32_t)g.sf, in_stride, out_stride);
        f.subtract = !dered_use_slopes(g.slope_doubles != 0, size, g.n_lo, (uint32_t)g.sf) ? RT_SUBTRACT_PER_SAMPLE
                     : dered_slope_vec(in, out, size, in_stride, out_stride)                 ? RT_SUBTRACT_SLOPE4
                                                                                             : RT_SUBTRACT_SLOPE1;
        if (f.fused) {   // deredden_slope_kernel<true>, norm_stats_finalize_kernel, norm_apply4_kernel in place
            f.norm_apply = RT_NORM_VEC;
            return f;
        }
        cur = out;
        cur_stride = out_stride;
    }
    if (normalise) {
        const bool vec = norm_vec_in(cur, cur_stride);
        f.norm_partial = vec ? RT_NORM_VEC : RT_NORM_SCALAR;
        f.norm_passes = (vec ? size / 4 : size) > kNormGridThreads ? 2 : 1;
        f.norm_apply = norm_vec_apply(cur, out, cur_stride, out_stride) ? RT_NORM_VEC : RT_NORM_SCALAR;
    }
    return f;
}

}  // namespace rt
