// The C ABI's host-only entry points: what the planner decides for a set of
// search parameters, read back without a device.  Each is checked_params ->
// planner (plan.hpp) -> copy out; rt_plan_create (capi_pgram.cpp) uploads the
// same plan_periodogram result.  Likewise the fold's shape and workspace
// (fold_host.hpp), the dereddening workspace (dered_host.hpp) and the candidate
// refinement's shift tables, specification and workspace (refine_host.hpp).  No HIP
// header (`make asan` builds this file as is).
#include "riptide_amd.h"

#include <algorithm>
#include <stdexcept>

#include "capi_common.hpp"
#include "dered_host.hpp"
#include "fold_host.hpp"
#include "peaks_host.hpp"
#include "plan.hpp"
#include "refine_host.hpp"

using namespace rt;

namespace {

PgramPlan pgram_plan(size_t size, double tsamp, double pmin, double pmax, size_t bmin, size_t bmax)
{
    PgramPlan pg;
    build_pgram_plan(checked_params(size, tsamp, pmin, pmax, bmin, bmax), pg);
    return pg;
}

// The host plan rt_plan_create builds for these parameters: wmax = the
// widest boxcar (0: unknown, as rt_schedule_check has no widths).
HostPlan host_plan(size_t size, double tsamp, size_t nw, uint32_t wmax, double pmin, double pmax, size_t bmin,
                   size_t bmax)
{
    HostPlan hp;
    plan_periodogram(checked_params(size, tsamp, pmin, pmax, bmin, bmax), (uint32_t)nw, wmax, scratch_budget_floats(),
                     cosched_banks(), hp);
    return hp;
}

}  // namespace

extern "C" {

const char* rt_last_error(void) { return last_error().c_str(); }

int rt_periodogram_length(size_t size, double tsamp, double pmin, double pmax, size_t bmin, size_t bmax,
                          size_t* length)
{
    return guarded([&] {
        *length = pgram_plan(size, tsamp, pmin, pmax, bmin, bmax).length;
        return RT_OK;
    });
}

int rt_periodogram_grid(size_t size, double tsamp, double pmin, double pmax, size_t bmin, size_t bmax,
                        double* periods, uint32_t* foldbins)
{
    return guarded([&] {
        fill_grid(pgram_plan(size, tsamp, pmin, pmax, bmin, bmax), periods, foldbins);
        return RT_OK;
    });
}

int rt_ffa_schedule_check(size_t rows, size_t cols, uint64_t* launches)
{
    return guarded([&] {
        if (!rows || !cols || rows > 0xFFFFFFFFull || cols > 0xFFFFFFFFull || !merge_slots((uint32_t)cols))
            throw std::invalid_argument("rt_ffa_schedule_check: bad shape");
        FfaXform X{};
        X.p = (uint32_t)cols;
        X.m = (uint32_t)rows;
        X.rows_eval = (uint32_t)rows;
        ExecPlan ex;
        build_exec_plan({X}, false, 0, ~0ull, ex);   // validates
        if (launches) *launches = ex.launches.size();
        return RT_OK;
    });
}

int rt_ladder_check(size_t size, double tsamp, double pmin, double pmax, size_t bmin, size_t bmax, int* fused,
                    uint64_t* rungs)
{
    return guarded([&] {
        const LadderPlan l = plan_ladder(pgram_plan(size, tsamp, pmin, pmax, bmin, bmax));
        if (fused) *fused = l.mode;
        if (rungs) *rungs = l.rungs.size();
        return RT_OK;
    });
}

int rt_ladder_layout(size_t size, double tsamp, double pmin, double pmax, size_t bmin, size_t bmax,
                     rt_ladder_rung* rungs, size_t cap, uint64_t* count, uint64_t* leaf_floats, int* mode,
                     uint32_t* margin)
{
    return guarded([&] {
        const PgramPlan pg = pgram_plan(size, tsamp, pmin, pmax, bmin, bmax);
        if (cap && !rungs) throw std::invalid_argument("rt_ladder_layout: rungs is NULL");
        const LadderPlan l = plan_ladder(pg);
        for (size_t i = 0; i < l.rungs.size() && i < cap; ++i) {
            const DsRung& d = l.rungs[i];
            rt_ladder_rung o{};
            o.f = d.f;
            o.n = d.n;
            o.leaf_off = d.out_off;
            o.fused = rung_in_fused(l.mode, d);
            rungs[i] = o;
        }
        if (count) *count = l.rungs.size();
        if (leaf_floats) *leaf_floats = pg.leaf_floats;
        if (mode) *mode = l.mode;
        if (margin) *margin = l.margin;
        return RT_OK;
    });
}

int rt_schedule_check(size_t size, double tsamp, size_t nw, double pmin, double pmax, size_t bmin, size_t bmax,
                      uint64_t* transforms, uint64_t* items, uint64_t* launches, double* alg_bytes,
                      double* moved_bytes, uint64_t* cells)
{
    return guarded([&] {
        const ExecTotals t = exec_totals(host_plan(size, tsamp, nw, 0, pmin, pmax, bmin, bmax).ex);
        *transforms = t.transforms;
        *items = t.items;
        *launches = t.launches;
        *alg_bytes = t.alg_bytes;
        *moved_bytes = t.moved_bytes;
        *cells = t.cells;
        return RT_OK;
    });
}

int rt_schedule_items(size_t size, double tsamp, size_t nw, double pmin, double pmax, size_t bmin, size_t bmax,
                      rt_schedule_item* items, size_t cap, uint64_t* count)
{
    return guarded([&] {
        if (cap && !items) throw std::invalid_argument("rt_schedule_items: items is NULL");
        const ExecPlan ex = host_plan(size, tsamp, nw, 0, pmin, pmax, bmin, bmax).ex;
        uint64_t n = 0;
        for (size_t l = 0; l < ex.launches.size(); ++l) {
            const Launch& L = ex.launches[l];
            for (uint32_t i = L.first; i < L.first + L.count; ++i, ++n) {
                if (n >= cap) continue;
                const ConeItem& it = ex.items[i];
                const FfaXform& X = ex.xf[it.xform];
                rt_schedule_item o{};
                o.launch = (uint32_t)l;
                o.pass = L.pass;
                o.slots = L.smax;
                o.snr_kind = L.snr;
                o.xform = it.xform;
                o.rung = X.rung;
                o.bins = X.p;
                o.node_start = it.node_start;
                o.node_size = it.node_size;
                o.s0 = it.s0;
                o.s1 = it.s1;
                o.levels = it.levels;
                o.src_leaves = it.src == kSelLeaves;
                o.tile = it.mode == kModeTile;
                items[n] = o;
            }
        }
        if (count) *count = n;
        return RT_OK;
    });
}

int rt_schedule_final_kinds(size_t size, double tsamp, const uint64_t* widths, size_t nw, double pmin, double pmax,
                            size_t bmin, size_t bmax, uint64_t* launches, uint64_t* rows_launches,
                            uint64_t* seg_launches, uint8_t* bins_kinds, size_t bins_cap)
{
    return guarded([&] {
        const uint32_t wmax = checked_plan_widths(widths, nw, bmin);
        const ExecPlan ex = host_plan(size, tsamp, nw, wmax, pmin, pmax, bmin, bmax).ex;
        uint64_t nr = 0, ns = 0;
        if (bins_kinds) std::fill(bins_kinds, bins_kinds + bins_cap, (uint8_t)0);
        for (const Launch& L : ex.launches) {
            if (L.snr == kSnrNone) continue;
            ++(L.snr == kSnrSeg ? ns : nr);
            if (!bins_kinds) continue;
            for (uint32_t i = L.first; i < L.first + L.count; ++i) {
                const uint32_t p = ex.xf[ex.items[i].xform].p;
                if (p < bins_cap) bins_kinds[p] |= (uint8_t)(L.snr == kSnrSeg ? 2 : 1);
            }
        }
        if (launches) *launches = ex.launches.size();
        if (rows_launches) *rows_launches = nr;
        if (seg_launches) *seg_launches = ns;
        return RT_OK;
    });
}

int rt_find_peaks_workspace_bytes(size_t batch, size_t length, size_t num_widths, size_t chunk_rows, size_t* bytes)
{
    return guarded([&] {
        *bytes = checked_peak_workspace(batch, length, num_widths, chunk_rows);
        return RT_OK;
    });
}

int rt_find_peaks_host(const float* snrs, size_t length, size_t num_widths, const double* logf, const double* freqs,
                       const double* coeffs, size_t ncoef, double smin, double radius, uint32_t* counts,
                       uint32_t* rows, float* snr, size_t cap)
{
    return guarded([&] {
        if (!cap) throw std::invalid_argument("rt_find_peaks_host: cap is 0");
        if (!ncoef || ncoef > 64) throw std::invalid_argument("rt_find_peaks_host: 1 to 64 polynomial coefficients");
        if (length >= (1ull << 32)) throw std::invalid_argument("rt_find_peaks_host: length must be below 2^32");
        for (size_t iw = 0; iw < num_widths; ++iw)
            counts[iw] = find_peaks_column(snrs + iw, num_widths, length, logf, freqs, coeffs + iw * ncoef,
                                           (uint32_t)ncoef, smin, radius, rows + iw * cap, snr + iw * cap, cap);
        return RT_OK;
    });
}

int rt_fold_shape(size_t size, double factor, size_t bins, size_t subints, size_t* m, size_t* rows)
{
    return guarded([&] {
        const FoldShape s = fold_shape(size, factor, bins, subints);
        if (m) *m = s.m;
        if (rows) *rows = s.rows;
        return RT_OK;
    });
}

int rt_fold_workspace_bytes(size_t size, const rt_fold_spec* specs, size_t nspecs, size_t* bytes)
{
    return guarded([&] {
        const size_t need = fold_plan(size, specs, nspecs).ws_bytes;
        if (bytes) *bytes = need;
        return RT_OK;
    });
}

int rt_refine_shifts(double period, double span, size_t bins, size_t subints, const double* band_freqs, size_t bands,
                     double dm, double kdm, const double* periods, size_t nper, const double* dms, size_t ndm,
                     int32_t* pshift, int32_t* dshift)
{
    return guarded([&] {
        refine_shifts(period, span, bins, subints, band_freqs, bands, dm, kdm, periods, nper, dms, ndm, pshift, dshift);
        return RT_OK;
    });
}

int rt_refine_host(const float* cube, size_t bands, size_t subints, size_t bins, const int32_t* dshift, size_t ndm,
                   const int32_t* pshift, size_t nper, const uint32_t* widths, size_t num_widths, float stdnoise,
                   float* snr, float* prof)
{
    return guarded([&] {
        refine_host(cube, bands, subints, bins, dshift, ndm, pshift, nper, widths, num_widths, stdnoise, snr, prof);
        return RT_OK;
    });
}

int rt_refine_workspace_bytes(const rt_refine_spec* specs, size_t nspecs, size_t* bytes)
{
    return guarded([&] {
        const size_t need = refine_plan(specs, nspecs).ws_bytes;
        if (bytes) *bytes = need;
        return RT_OK;
    });
}

int rt_deredden_workspace_bytes(size_t size, size_t ws, size_t minpts, size_t batch, size_t* bytes)
{
    return guarded([&] {
        *bytes = dered_ws_bytes(dered_geom(size, ws, minpts, batch, true));
        return RT_OK;
    });
}

int rt_deredden_forms(size_t size, size_t ws, size_t minpts, int deredden, int normalise, unsigned in_align,
                      unsigned out_align, size_t in_stride, size_t out_stride, rt_dered_forms* forms)
{
    return guarded([&] {
        if (!forms) throw std::invalid_argument("rt_deredden_forms: forms is NULL");
        if (in_align >= 16 || out_align >= 16 || in_align % 4 || out_align % 4)
            throw std::invalid_argument("rt_deredden_forms: an alignment is a float address mod 16");
        const DeredGeom g = dered_geom(size, ws, minpts, 1, deredden != 0);
        const DeredForms f =
            dered_forms(g, size, deredden != 0, normalise != 0, in_align, out_align, in_stride, out_stride);
        rt_dered_forms o{};
        o.scrunch_factor = g.sf;
        o.n_lo = g.n_lo;
        o.rmed_width = g.rmed_w;
        o.scrunch = f.scrunch;
        o.scrunch_chunks = f.scrunch_chunks;
        o.rmed = f.rmed;
        o.subtract = f.subtract;
        o.fused = f.fused;
        o.norm_partial = f.norm_partial;
        o.norm_passes = f.norm_passes;
        o.norm_apply = f.norm_apply;
        *forms = o;
        return RT_OK;
    });
}

}  // extern "C"
