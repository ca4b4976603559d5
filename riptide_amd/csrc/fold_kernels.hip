// Candidate folding for MI355X (gfx950): riptide/folding.py:19-81 over
// downsample.hpp:44-82 for a batch of candidates, device-resident.
//
//   fold_rows_kernel     the series downsampled by period / bins / tsamp, cut
//                        to whole periods and scaled: the (m, bins) row array
//   fold_subints_kernel  the row array summed to a profile, or downsampled
//                        along its first axis to the sub-integrations
//
// Exactness: the result is bit-identical to folding.fold -- every float
// operation of the reference on the same operands in the same order, with
// explicit *_rn intrinsics (no FMA contraction), no tree or cross-lane
// reductions.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "kernels.hpp"

namespace rt {

namespace {

constexpr uint32_t kFoldThreads = 256;

// wmin * w[0] + w[1] + ... + w[cnt - 1] added one by one in that order
// (downsample.hpp:75-77), elements `stride` floats apart (1: a window of the
// series; bins: a column of the row array).  The loads go out eight ahead of
// their additions; the elements past cnt - 1 of the last group add -0.0, an
// exact no-op.  The same scheme as window_sum of the ladder kernel.
__device__ __forceinline__ float fold_window_sum(const float* w, uint64_t stride, float wmin, uint32_t cnt)
{
    float acc = __fmul_rn(wmin, w[0]);
    uint32_t i = 1;
    for (; i + 8 <= cnt; i += 8) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = w[(uint64_t)(i + j) * stride];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, v[j]);
    }
    if (i < cnt) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = i + j < cnt ? w[(uint64_t)(i + j) * stride] : -0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, v[j]);
    }
    return acc;
}

// last entry of a first-block table that starts at or before block b
template <class First>
__device__ __forceinline__ uint32_t fold_find(uint32_t num, uint32_t b, First first)
{
    uint32_t lo = 0, hi = num - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (first(mid) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace

// One block = up to 256 consecutive outputs of one candidate's row array
// (fewer for large f, so the block's input span fits the LDS stage; 256
// outputs whose windows are read from global memory when f is too large to
// stage).  Candidates are flattened along blockIdx.x through their
// first-block table; each names its own series row.
__global__ __launch_bounds__(kFoldThreads) void fold_rows_kernel(
    const float* __restrict__ data, uint64_t n_in, const FoldCand* __restrict__ cands, uint32_t num_cands,
    float* __restrict__ out, float* __restrict__ rows_ws)
{
    __shared__ float span[kDsSpanFloats];
    const uint32_t b = blockIdx.x;
    const FoldCand c = cands[fold_find(num_cands, b, [&](uint32_t i) { return cands[i].first_block; })];
    const uint64_t k0 = (uint64_t)(b - c.first_block) * c.per_block;
    const uint64_t k1 = min(k0 + c.per_block, c.n_rows_out);
    const float* x = data + c.src_off;
    float* dst = (c.rows_in_ws ? rows_ws : out) + c.rows_off;
    const uint64_t k = k0 + threadIdx.x;
    const double f = c.f;
    const double last = (double)n_in - 1.0;
    // input span of the block: [imin(k0), imax(k1 - 1)]
    const uint64_t s0 = (uint64_t)floor(__dmul_rn((double)k0, f));
    double e1 = floor(__dadd_rn(__dmul_rn((double)(k1 - 1), f), f));
    if (e1 > last) e1 = last;
    const uint64_t s1 = (uint64_t)e1;
    const float* src = x + s0;
    if (c.staged) {
        const uint32_t len = (uint32_t)min(s1 - s0 + 1, (uint64_t)kDsSpanFloats);
        for (uint32_t i = threadIdx.x; i < len; i += kFoldThreads) span[i] = x[s0 + i];
        __syncthreads();
        src = span;
    }
    if (k >= k1) return;
    const double start = __dmul_rn((double)k, f);
    const double end = __dadd_rn(start, f);
    const uint64_t imin = (uint64_t)floor(start);
    double dmax = floor(end);
    if (dmax > last) dmax = last;
    const uint64_t imax = (uint64_t)dmax;
    const float wmin = (float)__dsub_rn((double)(imin + 1), start);
    const float wmax = (float)__dsub_rn(end, (double)imax);
    const float* w = src + (imin - s0);
    const uint32_t cnt = (uint32_t)(imax - imin);
    const float acc = __fadd_rn(fold_window_sum(w, 1, wmin, cnt), __fmul_rn(wmax, w[cnt]));
    dst[k] = __fmul_rn(acc, c.scale);
}

// One thread per output (s, b) of a candidate whose result is not the row
// array itself, b fastest (a wave reads consecutive floats of a row).
//   profile mode   out[b] = row[0][b] + row[1][b] + ... + row[m-1][b]
//                  (numpy's axis-0 sum of a C-contiguous float32 array)
//   vertical mode  out[s][b] = the downsample.hpp window sum of column b
//                  with factor vf = m / subints
// The two modes share no accumulation code: the profile starts from
// row[0][b] itself, the window from wmin * row[imin][b].
__global__ __launch_bounds__(kFoldThreads) void fold_subints_kernel(
    const FoldCand* __restrict__ cands, uint32_t num_cands, float* __restrict__ out,
    const float* __restrict__ rows_ws)
{
    const uint32_t blk = blockIdx.x;
    const FoldCand c = cands[fold_find(num_cands, blk, [&](uint32_t i) { return cands[i].first_block; })];
    const uint64_t idx = (uint64_t)(blk - c.first_block) * kFoldThreads + threadIdx.x;
    const uint64_t bins = c.bins;
    if (idx >= (uint64_t)c.sub_rows * bins) return;
    const uint64_t s = idx / bins;
    const uint64_t col = idx - s * bins;
    const float* rows = rows_ws + c.rows_off + col;
    float* dst = out + c.out_off;
    if (c.mode == kFoldProfile) {
        float acc = rows[0];
        uint32_t i = 1;
        const uint32_t m = c.m;
        for (; i + 8 <= m; i += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = rows[(uint64_t)(i + j) * bins];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = __fadd_rn(acc, v[j]);
        }
        for (; i < m; ++i) acc = __fadd_rn(acc, rows[(uint64_t)i * bins]);
        dst[col] = acc;
        return;
    }
    const double vf = c.vf;
    const double last = (double)c.m - 1.0;
    const double start = __dmul_rn((double)s, vf);
    const double end = __dadd_rn(start, vf);
    const uint64_t imin = (uint64_t)floor(start);
    double dmax = floor(end);
    if (dmax > last) dmax = last;
    const uint64_t imax = (uint64_t)dmax;
    const float wmin = (float)__dsub_rn((double)(imin + 1), start);
    const float wmax = (float)__dsub_rn(end, (double)imax);
    const float* w = rows + imin * bins;
    const uint32_t cnt = (uint32_t)(imax - imin);
    dst[idx] = __fadd_rn(fold_window_sum(w, bins, wmin, cnt), __fmul_rn(wmax, w[(uint64_t)cnt * bins]));
}

hipError_t launch_fold_rows(const float* data, uint64_t n_in, const FoldCand* d_cands, uint32_t num_cands,
                            uint32_t total_blocks, float* out, float* rows_ws, hipStream_t s)
{
    if (!num_cands || !total_blocks) return hipSuccess;
    hipLaunchKernelGGL(fold_rows_kernel, dim3(total_blocks), dim3(kFoldThreads), 0, s, data, n_in, d_cands,
                       num_cands, out, rows_ws);
    return hipGetLastError();
}

hipError_t launch_fold_subints(const FoldCand* d_cands, uint32_t num_cands, uint32_t total_blocks, float* out,
                               const float* rows_ws, hipStream_t s)
{
    if (!num_cands || !total_blocks) return hipSuccess;
    hipLaunchKernelGGL(fold_subints_kernel, dim3(total_blocks), dim3(kFoldThreads), 0, s, d_cands, num_cands, out,
                       rows_ws);
    return hipGetLastError();
}

}  // namespace rt
