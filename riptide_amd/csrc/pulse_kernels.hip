// Single-pulse search on the device (pulse_host.hpp has the specification and
// the summation order this file reproduces bit for bit).
//
//   pulse_tile_kernel: one workgroup of 1024 threads per (tile of kPulseTile
//     outputs, series).  The tile's outputs and a halo of `radius` on each side
//     are worked through in chunks: a chunk's samples (with the largest width
//     around them, from the start of the segment the first one lies in) are
//     read once, a wave per segment of 1024, a lane per run of 16, and their
//     float64 partial sums written to LDS, 17 slots per run (slot 0: the run's
//     base, slot i: the sum through sample i - 1; the odd stride keeps the 16
//     lanes of a ds_write_b64 group and the 32 lanes of a ds_read_b64 group on
//     distinct banks).  Every output of the chunk then takes its K window sums
//     from two slots each (and the totals of the segments between), divides,
//     and keeps the centred best in LDS.  With every chunk done the tile's
//     samples are tested against their neighbours within the radius, the
//     events numbered in sample order (ballots, wave counts) and written to a
//     run of the pool claimed by one atomic add per tile.
//   pulse_offsets_kernel: the exclusive sum of the tiles' counts in (series,
//     tile) order, and the total.
//   pulse_gather_kernel: every tile's run copied from the pool to its place in
//     the list.  The order in which tiles claimed the pool does not show.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "pulse_kernels.hpp"

namespace rt {

namespace {

constexpr int kT = (int)kPulseTile;
constexpr int kS = (int)kPulseSeg;
constexpr int kSlots = (int)kPulseSegSlots;
constexpr int kThreads = (int)kPulseThreads;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = kT / kThreads;
static_assert(kWaves * kIters <= 64, "the wave counts of a tile");

__global__ __launch_bounds__(kThreads) void pulse_tile_kernel(PulseArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char pulse_lds[];
    double* F = reinterpret_cast<double*>(pulse_lds);
    float* bbuf = reinterpret_cast<float*>(F + (size_t)A.chunk_segs * kSlots);
    int16_t* kbuf = reinterpret_cast<int16_t*>(bbuf + A.best_floats);
    uint32_t* wcnt = reinterpret_cast<uint32_t*>(kbuf + kT);
    unsigned long long* sbase = reinterpret_cast<unsigned long long*>(wcnt + 64);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t tile = blockIdx.x, b = blockIdx.y;
    const int N = (int)A.N, R = (int)A.R, wmax = (int)A.wmax, cmax = wmax >> 1, chunk = (int)A.chunk;
    const int t0 = (int)tile * kT, t1 = min(N, t0 + kT);
    const int e0 = t0 - R;                        // the sample of bbuf[0]
    const int ext_lo = max(0, e0), ext_hi = min(N, t1 + R);
    const float* __restrict__ xr = A.x + (uint64_t)b * A.ldx;

    for (int cu = ext_lo; cu < ext_hi; cu += chunk) {
        const int ce = min(cu + chunk, ext_hi);
        const int lo_s = max(0, cu - cmax) / kS * kS;
        const int hi_s = min(N, ce - 1 - cmax + wmax);
        const int nseg = min((hi_s - lo_s + kS - 1) / kS, (int)A.chunk_segs);
        __syncthreads();   // the chunk before is read
        for (int seg = wave; seg < nseg; seg += kWaves) {
            const int g = lo_s + seg * kS + (int)kPulseRun * lane;
            double r[kPulseRun];
#pragma unroll
            for (int i = 0; i < (int)kPulseRun; ++i) {
                const double v = g + i < N ? (double)xr[g + i] : 0.0;
                r[i] = i ? r[i - 1] + v : v;
            }
            const double tot = r[kPulseRun - 1];
            double base = 0.0;
            for (int j = 0; j < 63; ++j) {
                const double tj = __shfl(tot, j);
                if (j < lane) base = base + tj;
            }
            double* Fs = F + seg * kSlots + ((int)kPulseRun + 1) * lane;
            Fs[0] = base;
#pragma unroll
            for (int i = 0; i < (int)kPulseRun; ++i) Fs[i + 1] = base + r[i];
        }
        __syncthreads();
        for (int u = cu + tid; u < ce; u += kThreads) {
            float bv = -INFINITY;
            int bk = -1;
            for (uint32_t k = 0; k < A.K; ++k) {
                const PulseWidth pw = A.widths[k];
                const int a = u - pw.c, e = a + pw.w;
                if (a < 0 || e > N) continue;
                const int ra = a - lo_s, re = e - 1 - lo_s;
                const double Ea = F[ra + (ra >> 4)];
                const double Ie = F[re + (re >> 4) + 1];
                const int ga = ra / kS, ge = re / kS;
                double d;
                if (ga == ge) {
                    d = Ie - Ea;
                } else {
                    double acc = F[ga * kSlots + kSlots - 1] - Ea;
                    for (int gg = ga + 1; gg < ge; ++gg) acc = acc + F[gg * kSlots + kSlots - 1];
                    d = acc + Ie;
                }
                const float s = (float)(d / pw.sq);
                if (s > bv) {
                    bv = s;
                    bk = (int)k;
                }
            }
            bbuf[u - e0] = bv;
            if (u >= t0 && u < t1) {
                kbuf[u - t0] = (int16_t)bk;
                const uint64_t at = (uint64_t)b * A.N + (uint32_t)u;
                if (A.best) A.best[at] = bv;
                if (A.kbest) A.kbest[at] = bk;
            }
        }
    }
    __syncthreads();

    // the neighbourhood rule, then the tile's events in sample order
    const uint64_t below = (1ull << lane) - 1;
    uint32_t evbits = 0, rank[kIters];
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int t = t0 + it * kThreads + tid;
        bool ev = false;
        if (t < t1) {
            const float v = bbuf[t - e0];
            if (v >= A.threshold) {
                ev = true;
                for (int u = max(0, t - R); u < t; ++u)
                    if (!(v > bbuf[u - e0])) {
                        ev = false;
                        break;
                    }
                if (ev) {
                    const int hi = min(N - 1, t + R);
                    for (int u = t + 1; u <= hi; ++u)
                        if (!(v >= bbuf[u - e0])) {
                            ev = false;
                            break;
                        }
                }
            }
        }
        const uint64_t mask = __ballot(ev);
        if (lane == 0) wcnt[it * kWaves + wave] = (uint32_t)__builtin_popcountll(mask);
        rank[it] = (uint32_t)__builtin_popcountll(mask & below);
        evbits |= (uint32_t)ev << it;
    }
    __syncthreads();
    const uint64_t tidx = (uint64_t)b * gridDim.x + tile;
    if (tid == 0) {
        uint32_t total = 0;
        for (int i = 0; i < kIters * kWaves; ++i) {
            const uint32_t c = wcnt[i];
            wcnt[i] = total;
            total += c;
        }
        unsigned long long pos = 0;
        if (total) pos = atomicAdd(A.cursor, (unsigned long long)total);
        *sbase = pos;
        A.tile_cnt[tidx] = total;
        A.tile_pos[tidx] = pos;
    }
    __syncthreads();
    const unsigned long long pos = *sbase;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        if (!(evbits >> it & 1)) continue;
        const int t = t0 + it * kThreads + tid;
        const unsigned long long at = pos + wcnt[it * kWaves + wave] + rank[it];
        if (at < A.cap) A.pool[at] = rt_pulse_event{(int32_t)b, t, (int32_t)kbuf[t - t0], bbuf[t - e0]};
    }
}

__global__ __launch_bounds__(1024) void pulse_offsets_kernel(const uint32_t* __restrict__ cnt, uint32_t ntiles,
                                                             uint64_t* __restrict__ off, uint64_t* __restrict__ count)
{
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ntiles + 1023) / 1024;
    const uint32_t i0 = (uint32_t)min((uint64_t)tid * per, (uint64_t)ntiles), i1 = min(i0 + per, ntiles);
    uint64_t sum = 0;
    for (uint32_t i = i0; i < i1; ++i) sum += cnt[i];
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 1024; ++i) {
            const uint64_t c = part[i];
            part[i] = run;
            run += c;
        }
        *count = run;
    }
    __syncthreads();
    uint64_t run = part[tid];
    for (uint32_t i = i0; i < i1; ++i) {
        off[i] = run;
        run += cnt[i];
    }
}

__global__ __launch_bounds__(256) void pulse_gather_kernel(const uint32_t* __restrict__ cnt,
                                                           const uint64_t* __restrict__ pos,
                                                           const uint64_t* __restrict__ off, uint32_t ntiles,
                                                           const rt_pulse_event* __restrict__ pool,
                                                           rt_pulse_event* __restrict__ events, uint64_t cap)
{
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= ntiles) return;
    const uint32_t n = cnt[i];
    const uint64_t from = pos[i], to = off[i];
    for (uint32_t k = lane; k < n; k += 64)
        if (from + k < cap && to + k < cap) events[to + k] = pool[from + k];
}

}  // namespace

hipError_t launch_single_pulse(const PulseArgs& A, uint32_t nseries, uint32_t lds_bytes, uint64_t* tile_off,
                               rt_pulse_event* d_events, uint64_t* d_count, hipStream_t s)
{
    if (!nseries || !A.tiles) return hipSuccess;
    if (lds_bytes > kPulseLdsMax) return hipErrorInvalidValue;
    {
        // > 64 KiB of dynamic LDS: opt in once per device
        static std::mutex mu;
        static uint64_t done = 0;   // bit d: device d opted in
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        std::lock_guard<std::mutex> lk(mu);
        if (dev >= 64 || !(done >> dev & 1)) {
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(pulse_tile_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPulseLdsMax);
            if (e != hipSuccess) return e;
            if (dev < 64) done |= 1ull << dev;
        }
    }
    const uint32_t ntiles = nseries * A.tiles;
    hipLaunchKernelGGL(pulse_tile_kernel, dim3(A.tiles, nseries), dim3(kThreads), lds_bytes, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pulse_offsets_kernel, dim3(1), dim3(1024), 0, s, A.tile_cnt, ntiles, tile_off, d_count);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (A.cap)
        hipLaunchKernelGGL(pulse_gather_kernel, dim3((ntiles + 3) / 4), dim3(256), 0, s, A.tile_cnt, A.tile_pos,
                           tile_off, ntiles, A.pool, d_events, A.cap);
    return hipGetLastError();
}

}  // namespace rt
