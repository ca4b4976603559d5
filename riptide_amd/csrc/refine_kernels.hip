// Candidate refinement for MI355X (gfx950): the shift-and-add search over DM
// and period offsets of refine_host.hpp for a batch of folded cubes.
//
// Both stages are one operation, "stage a slice of R rows x N bins, then for
// every trial t sum the rows rotated by shift[t][r]", and one kernel:
//
//   stage A  refine_kernel<false>  block = (candidate, sub-integration s):
//            the slice x[:, s, :] (bands x bins), a trial per DM, each result
//            row written to y[k][s][:] in the workspace
//   stage B  refine_kernel<true>   block = (candidate, DM trial k): the slice
//            y[k] (subints x bins), a trial per period, each profile's boxcar
//            S/N (and the profile itself when asked) written out
//
// A slice of at most kRefineStageBytes is staged in LDS (every element is then
// fetched from memory once per block and the rotated reads are LDS reads of
// consecutive addresses); a larger one is read from global memory by the same
// code.  Exactness: a profile is bit-identical to refine_host -- each sum starts
// from 0.0f and adds its terms in index order with __fadd_rn, one lane per
// bin, no tree or cross-lane reduction -- whichever path a slice takes.
//
// No table entry can cause a read outside the slice: a shift is reduced by an
// unsigned modulo as the table is loaded (once per row of a trial, into LDS), a
// width is clamped to [1, bins - 1].
#include <hip/hip_runtime.h>

#include <mutex>

#include "common.hpp"
#include "kernels.hpp"

namespace rt {

namespace {

__device__ __forceinline__ double refine_wave_scan(double v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

__device__ __forceinline__ float refine_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// last candidate whose first block is at or before block b
template <bool kSnr>
__device__ __forceinline__ uint32_t refine_find(const RefineCand* cands, uint32_t num, uint32_t b)
{
    uint32_t lo = 0, hi = num - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if ((kSnr ? cands[mid].first_b : cands[mid].first_a) <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The block's LDS, carved from one dynamic array (RefinePlan::lds_a / lds_b bytes).
struct RefineLds {
    double* wtot;     // 4 wave totals of the prefix sum
    float* prof;      // kRefineMaxBins
    float* cps;       // kRefineMaxBins
    uint32_t* sh;     // 2 x kRefineThreads reduced shifts
    float* stage;     // the slice
};

// Boxcar S/N of the profile in L.prof (snr.hpp:37-55): fp64 prefix sums across
// the block, then a wave per width.  Called by every thread of the block.
__device__ __forceinline__ void refine_snr(const RefineLds& L, uint32_t N, const uint32_t* __restrict__ widths,
                                           uint32_t W, float stdnoise, float* __restrict__ out)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t cs = (N + kRefineThreads - 1) / kRefineThreads;
    const uint32_t j0 = min(tid * cs, N), j1 = min(j0 + cs, N);
    double part = 0.0;
    for (uint32_t j = j0; j < j1; ++j) part += (double)L.prof[j];
    const double incl = refine_wave_scan(part, (int)lane);
    if (lane == 63) L.wtot[wave] = incl;
    __syncthreads();
    double acc = incl - part;
    for (uint32_t v = 0; v < wave; ++v) acc += L.wtot[v];
    for (uint32_t j = j0; j < j1; ++j) {
        acc += (double)L.prof[j];
        L.cps[j] = (float)acc;
    }
    __syncthreads();
    const float sum = L.cps[N - 1];
    for (uint32_t iw = wave; iw < W; iw += kRefineThreads / 64) {
        const uint32_t w = min(max(widths[iw], 1u), N - 1);
        float dmax = -INFINITY;
        for (uint32_t i = lane; i < N; i += 64) {
            const uint32_t k = i + w;
            const float ck = k < N ? L.cps[k] : __fadd_rn(L.cps[k - N], sum);
            dmax = fmaxf(dmax, __fsub_rn(ck, L.cps[i]));
        }
        dmax = refine_wave_max(dmax);
        if (lane == 0) {
            const float h = sqrtf((float)(N - w) / (float)(N * w));
            const float b = (float)w / (float)(N - w) * h;
            out[iw] = ((h + b) * dmax - b * sum) / stdnoise;
        }
    }
}

// Every trial of the block: rows[r * rstride + n] is the slice (LDS or global
// memory), tab[t * R + r] the trial's shifts.  A thread owns bins tid, tid +
// 256, ... (E of them: E = ceil(N / 256)); a lane past N in the last group
// works on bin 0 and stores nothing.
//   kSnr false: out_rows[t * out_stride + n] = the sum
//   kSnr true : the sum is trial t's profile: its S/N to snr[t * W + w], itself
//               to profiles[t * N + n] unless that is null
template <bool kSnr, int E, class Rows>
__device__ __forceinline__ void refine_trials(const RefineLds& L, Rows rows, uint64_t rstride, uint32_t R, uint32_t N,
                                              const int32_t* __restrict__ tab, uint32_t T,
                                              float* __restrict__ out_rows, uint64_t out_stride,
                                              const uint32_t* __restrict__ widths, uint32_t W, float stdnoise,
                                              float* __restrict__ snr, float* __restrict__ profiles)
{
    const uint32_t tid = threadIdx.x;
    const bool last_ok = tid + (E - 1) * kRefineThreads < N;
    uint32_t n[E];
#pragma unroll
    for (int i = 0; i < E; ++i) n[i] = tid + i * kRefineThreads;
    if (!last_ok) n[E - 1] = 0;
    uint32_t parity = 0;
    for (uint32_t t = 0; t < T; ++t) {
        float acc[E];
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] = 0.0f;
        for (uint32_t r0 = 0; r0 < R; r0 += kRefineThreads) {
            // the chunk's shifts, reduced once each.  Two buffers: a thread may
            // load the next chunk while others still read this one; the
            // barrier of that next chunk separates them from the one after.
            uint32_t* sh = L.sh + parity * kRefineThreads;
            parity ^= 1;
            if (r0 + tid < R) sh[tid] = (uint32_t)tab[(uint64_t)t * R + r0 + tid] % N;
            __syncthreads();
            const uint32_t rc = min(kRefineThreads, R - r0);
            Rows row = rows + (uint64_t)r0 * rstride;
#pragma unroll 4
            for (uint32_t r = 0; r < rc; ++r, row += rstride) {
                const uint32_t d = sh[r];
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    uint32_t q = n[i] + d;
                    q = q >= N ? q - N : q;
                    acc[i] = __fadd_rn(acc[i], row[q]);
                }
            }
        }
        if (!kSnr) {
            float* dst = out_rows + (uint64_t)t * out_stride;
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i < E - 1 || last_ok) dst[n[i]] = acc[i];
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i < E - 1 || last_ok) {
                    L.prof[n[i]] = acc[i];
                    if (profiles) profiles[(uint64_t)t * N + n[i]] = acc[i];
                }
            __syncthreads();
            refine_snr(L, N, widths, W, stdnoise, snr + (uint64_t)t * W);
        }
    }
}

template <bool kSnr, class Rows>
__device__ __forceinline__ void refine_dispatch(const RefineLds& L, Rows rows, uint64_t rstride, uint32_t R, uint32_t N,
                                                const int32_t* tab, uint32_t T, float* out_rows, uint64_t out_stride,
                                                const uint32_t* widths, uint32_t W, float stdnoise, float* snr,
                                                float* profiles)
{
    switch ((N + kRefineThreads - 1) / kRefineThreads) {
    case 1: refine_trials<kSnr, 1>(L, rows, rstride, R, N, tab, T, out_rows, out_stride, widths, W, stdnoise, snr, profiles); break;
    case 2: refine_trials<kSnr, 2>(L, rows, rstride, R, N, tab, T, out_rows, out_stride, widths, W, stdnoise, snr, profiles); break;
    case 3: refine_trials<kSnr, 3>(L, rows, rstride, R, N, tab, T, out_rows, out_stride, widths, W, stdnoise, snr, profiles); break;
    default: refine_trials<kSnr, 4>(L, rows, rstride, R, N, tab, T, out_rows, out_stride, widths, W, stdnoise, snr, profiles); break;
    }
}

}  // namespace

template <bool kSnr>
__global__ __launch_bounds__(kRefineThreads) void refine_kernel(
    const float* __restrict__ cubes, const int32_t* __restrict__ shifts, const uint32_t* __restrict__ widths,
    const RefineCand* __restrict__ cands, uint32_t num_cands, float* __restrict__ y, float* __restrict__ snr,
    float* __restrict__ profiles)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char refine_lds[];
    RefineLds L;
    L.wtot = (double*)refine_lds;
    L.prof = (float*)(refine_lds + 32);
    L.cps = L.prof + kRefineMaxBins;
    L.sh = (uint32_t*)(L.cps + kRefineMaxBins);
    L.stage = (float*)(L.sh + 2 * kRefineThreads);

    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const RefineCand c = cands[refine_find<kSnr>(cands, num_cands, blk)];
    const uint32_t u = blk - (kSnr ? c.first_b : c.first_a);   // stage A: s; stage B: k
    const uint32_t N = c.bins, S = c.subints;
    const uint32_t R = kSnr ? S : c.bands;
    const uint32_t T = kSnr ? c.nper : c.ndm;
    // the slice's rows: x[r][u][:] (stage A), y[u][r][:] (stage B)
    const float* src = kSnr ? y + c.y_off + (uint64_t)u * S * N : cubes + c.cube_off + (uint64_t)u * N;
    const uint64_t rstride = kSnr ? (uint64_t)N : (uint64_t)S * N;
    const int32_t* tab = shifts + (kSnr ? c.pshift_off : c.dshift_off);
    float* out_rows = kSnr ? nullptr : y + c.y_off + (uint64_t)u * N;   // y[t][u][:], t stride S * N
    const uint64_t out_stride = (uint64_t)S * N;
    const uint32_t* wd = widths + c.width_off;
    float* so = kSnr ? snr + c.snr_off + (uint64_t)u * c.nper * c.nw : nullptr;
    float* po = (kSnr && profiles) ? profiles + c.prof_off + (uint64_t)u * c.nper * N : nullptr;

    if (kSnr ? c.staged_b : c.staged_a) {
        const uint32_t total = R * N;   // <= kRefineStageBytes / 4
        for (uint32_t e = tid; e < total; e += kRefineThreads) {
            const uint32_t r = e / N;
            L.stage[e] = src[(uint64_t)r * rstride + (e - r * N)];
        }
        // (the first chunk's barrier in refine_trials orders these writes before the reads)
        refine_dispatch<kSnr>(L, (const float*)L.stage, (uint64_t)N, R, N, tab, T, out_rows, out_stride, wd, c.nw,
                              c.stdnoise, so, po);
    } else {
        refine_dispatch<kSnr>(L, src, rstride, R, N, tab, T, out_rows, out_stride, wd, c.nw, c.stdnoise, so, po);
    }
}

namespace {

// more than 64 KiB of dynamic LDS: opt in once per device and kernel
template <bool kSnr>
hipError_t refine_opt_in()
{
    static std::mutex mu;
    static uint64_t done = 0;   // bit d: device d opted in
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 64 || !(done >> dev & 1)) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(refine_kernel<kSnr>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(kRefineFixedLds + kRefineStageBytes));
        if (e != hipSuccess) return e;
        if (dev < 64) done |= 1ull << dev;
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_refine(const float* d_cubes, const int32_t* d_shifts, const uint32_t* d_widths,
                         const RefineCand* d_cands, uint32_t num_cands, uint32_t blocks_a, uint32_t blocks_b,
                         uint32_t lds_a, uint32_t lds_b, float* d_y, float* d_snr, float* d_profiles, hipStream_t s)
{
    if (!num_cands || !blocks_a || !blocks_b) return hipSuccess;
    if (lds_a > kRefineFixedLds + kRefineStageBytes || lds_b > kRefineFixedLds + kRefineStageBytes)
        return hipErrorInvalidValue;
    hipError_t e = refine_opt_in<false>();
    if (e != hipSuccess) return e;
    e = refine_opt_in<true>();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refine_kernel<false>, dim3(blocks_a), dim3(kRefineThreads), lds_a, s, d_cubes, d_shifts,
                       d_widths, d_cands, num_cands, d_y, d_snr, d_profiles);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refine_kernel<true>, dim3(blocks_b), dim3(kRefineThreads), lds_b, s, d_cubes, d_shifts,
                       d_widths, d_cands, num_cands, d_y, d_snr, d_profiles);
    return hipGetLastError();
}

}  // namespace rt
