// Host planning of the batched candidate fold (folding.py:19-81): a
// candidate's shape, the descriptor tables of one call, the workspace layout
// and the result-range check.  No HIP header: shared by the kernels'
// declarations (kernels.hpp), the C ABI (capi_fold.cpp, host_api.cpp) and the
// sanitizer checker (host_check_main.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "capi_common.hpp"
#include "common.hpp"
#include "plan.hpp"

namespace rt {

// What a candidate's result is: the (m, bins) row array itself, its sum over
// the rows, or the row array downsampled along its first axis.
constexpr uint32_t kFoldRows = 0, kFoldProfile = 1, kFoldVertical = 2;

// One candidate of a batched fold.  The same descriptor serves both kernels:
// first_block is the candidate's first block of the launch the table belongs
// to (the rows table holds every candidate, the subints table those whose
// mode is not kFoldRows).
struct FoldCand {
    double f;             // period / bins / tsamp
    double vf;            // kFoldVertical: m / subints
    uint64_t src_off;     // float offset of the candidate's series in d_data
    uint64_t n_rows_out;  // m * bins
    uint64_t rows_off;    // float offset of the row array: in d_out (kFoldRows) or in the workspace rows
    uint64_t out_off;     // float offset of the result in d_out
    float scale;          // (float)pow(m * f, -0.5)
    uint32_t bins;
    uint32_t m;           // whole periods
    uint32_t sub_rows;    // rows of the subints kernel's output (1 for a profile)
    uint32_t mode;
    uint32_t rows_in_ws;
    uint32_t first_block;
    uint32_t per_block;   // rows kernel: outputs per block (ds_per_block, or 256 unstaged)
    uint32_t staged;      // rows kernel: the block's input span is staged in LDS
    uint32_t pad;
};

// m and the mode / result rows of one candidate; throws as the header lists.
struct FoldShape {
    uint64_t m = 0;
    uint32_t mode = kFoldRows;
    uint64_t rows = 0;      // result rows (0: a 1-D profile)
    double vf = 0.0;
};

inline FoldShape fold_shape(size_t size, double f, size_t bins, size_t subints)
{
    if (!((f > 1.0) & (f <= (double)size)))
        throw std::invalid_argument("Downsampling factor must verify: 1 < f <= size");
    if (bins < 2) throw std::invalid_argument("fold: bins must be >= 2");
    if (bins > 0xFFFFFFFFull) throw std::invalid_argument("fold: too many bins");
    FoldShape s;
    s.m = downsampled_size(size, f) / bins;
    if (!s.m) throw std::invalid_argument("fold: no whole period fits in the data");
    if (s.m > 0xFFFFFFFFull) throw std::invalid_argument("fold: too many periods");
    if (subints > s.m) throw std::invalid_argument("fold: subints exceeds the number of whole periods");
    if (subints == 1 || s.m == 1) {
        s.mode = kFoldProfile;
    } else if (subints == 0 || subints == s.m) {
        s.rows = s.m;
    } else {
        s.mode = kFoldVertical;
        s.vf = (double)s.m / (double)subints;
        s.rows = downsampled_size(s.m, s.vf);
    }
    return s;
}

// The launch plan of one call: the rows table (every candidate), the subints
// table (those whose result is not the row array) and the workspace layout
// [both tables | row arrays of the subints candidates].
struct FoldPlan {
    std::vector<FoldCand> rows, sub;
    uint32_t rows_blocks = 0, sub_blocks = 0;
    size_t table_bytes = 0, ws_bytes = 0;
};

// (static: a signature naming the C ABI's struct stays out of the library's
// dynamic symbols)
static inline FoldPlan fold_plan(size_t size, const rt_fold_spec* specs, size_t nspecs)
{
    FoldPlan P;
    if (!nspecs) return P;
    if (!specs) throw std::invalid_argument("fold: null specs");
    uint64_t rb = 0, sb = 0, ws_floats = 0;
    P.rows.reserve(nspecs);
    for (size_t i = 0; i < nspecs; ++i) {
        const rt_fold_spec& sp = specs[i];
        const FoldShape sh = fold_shape(size, sp.factor, sp.bins, sp.subints);
        FoldCand c{};
        c.f = sp.factor;
        c.vf = sh.vf;
        c.n_rows_out = sh.m * (uint64_t)sp.bins;
        c.out_off = sp.out_off;
        c.scale = (float)std::pow((double)sh.m * sp.factor, -0.5);
        c.bins = sp.bins;
        c.m = (uint32_t)sh.m;
        c.mode = sh.mode;
        c.sub_rows = sh.mode == kFoldProfile ? 1u : (uint32_t)sh.rows;
        c.rows_in_ws = sh.mode != kFoldRows;
        c.rows_off = c.rows_in_ws ? ws_floats : sp.out_off;
        const uint32_t o = ds_per_block(sp.factor);
        c.staged = o >= 32;
        c.per_block = c.staged ? o : 256u;
        c.first_block = (uint32_t)rb;
        rb += (c.n_rows_out + c.per_block - 1) / c.per_block;
        if (rb > 0x7FFFFFFFull) throw std::invalid_argument("fold: too many outputs for one call");
        P.rows.push_back(c);
        if (c.rows_in_ws) {
            ws_floats += c.n_rows_out;
            FoldCand d = c;
            d.first_block = (uint32_t)sb;
            sb += ((uint64_t)c.sub_rows * c.bins + 255) / 256;
            P.sub.push_back(d);
        }
    }
    P.rows_blocks = (uint32_t)rb;
    P.sub_blocks = (uint32_t)sb;
    P.table_bytes = align_up((P.rows.size() + P.sub.size()) * sizeof(FoldCand), 256);
    P.ws_bytes = P.table_bytes + ws_floats * sizeof(float);
    return P;
}

inline size_t fold_result_floats(const FoldCand& c)
{
    return c.mode == kFoldRows ? c.n_rows_out : (size_t)c.sub_rows * c.bins;
}

// series indices, result ranges inside out_floats and disjoint
static inline void fold_check_ranges(const FoldPlan& P, const rt_fold_spec* specs, size_t nseries, size_t out_floats)
{
    std::vector<std::pair<uint64_t, uint64_t>> rng;
    rng.reserve(P.rows.size());
    for (size_t i = 0; i < P.rows.size(); ++i) {
        if (specs[i].series >= nseries) throw std::invalid_argument("fold: series index out of range");
        const uint64_t lo = P.rows[i].out_off, len = fold_result_floats(P.rows[i]);
        if (lo > out_floats || len > out_floats - lo)
            throw std::invalid_argument("fold: result range exceeds the output buffer");
        rng.emplace_back(lo, lo + len);
    }
    std::sort(rng.begin(), rng.end());
    for (size_t i = 1; i < rng.size(); ++i)
        if (rng[i].first < rng[i - 1].second) throw std::invalid_argument("fold: result ranges overlap");
}

}  // namespace rt
