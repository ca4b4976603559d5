// Host geometry of dereddening + normalisation: the scrunch factor and the
// running-median width of a call, and the layout of its device workspace
// [lores | rmed | slopes | partials].  No HIP header.
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

}  // namespace rt
