// Signal injection for MI355X (gfx950): the specification of inject_host.hpp,
// in place on a device-resident block, one pass.
//
//   inject_kernel<SPD>   1-D grid of (dword-column block, tile of super-rows).
//                        SPD = 4: an 8-bit block, a lane owns one aligned
//                        dword = four samples; SPD = 1: a float32 block, a
//                        lane owns one float.
//
// Layout.  Lanes run along the channel axis.  A super-row is SPD rows =
// nchans dwords for every nchans, so the block is an array [super-row][nchans]
// of aligned dwords (counted from the aligned address at or below a
// misaligned 8-bit block) and a lane that walks down its dword column keeps
// the same (row within the super-row, channel) for each of its SPD samples.
// It reads their delays and amplitudes once per signal and reuses them over
// the kInjectLaneSamples / SPD super-rows it walks.  The signals are the outer
// loop, the rows the inner one, with one accumulator per sample in registers:
// every sample adds its signals in table order, as the specification does.
// Every dword wholly inside the block is read and written as a dword; only
// the dwords that straddle the first or the last byte of a misaligned or
// ragged 8-bit block (at most two per call) go byte by byte, so nothing
// outside the block is read or written.
//
// A periodic signal without acceleration advances its phase by SPD * step per
// super-row: one 64-bit add per sample, no multiply and no float64.  The
// factor of a signal is wave-uniform (the table is read through scalar
// loads), so the branch to the float64 path costs an unaccelerated signal
// nothing.  Templates are gathered from global memory through the cache: a
// table of 2^10 floats is 4 KiB.  The float32 product and sums are
// __fmul_rn / __fadd_rn (and the build's -ffp-contract=off): no FMA.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rt {

namespace {

// inject_time of inject_host.hpp
__device__ __forceinline__ int64_t inject_time_dev(double f, uint64_t span, int64_t u)
{
    const int64_t q = (int64_t)((uint64_t)u * (span - (uint64_t)u));
    const int64_t s = (int64_t)rint(f * (double)q);
    return (int64_t)((uint64_t)u + (uint64_t)s);
}

__device__ __forceinline__ float inject_dither_dev(uint64_t t, uint32_t nchans, uint32_t c, uint64_t salt)
{
    uint64_t z = t * nchans + c + salt;
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(uint32_t)(z >> 40) * 0x1p-24f;
}

__device__ __forceinline__ int32_t inject_increment_dev(float acc, float r)
{
    return (int32_t)floorf(fminf(fmaxf(__fadd_rn(acc, r), -65536.0f), 65536.0f));
}

template <bool SIGNED>
__device__ __forceinline__ uint32_t inject_byte(uint32_t byte, int32_t d)
{
    if (SIGNED) return (uint32_t)min(max((int32_t)(int8_t)byte + d, -128), 127) & 0xffu;
    return (uint32_t)min(max((int32_t)byte + d, 0), 255);
}

template <uint32_t SPD, bool SIGNED>
__global__ __launch_bounds__(kInjectThreads) void inject_kernel(InjectArgs A)
{
    constexpr uint32_t ROWS = kInjectLaneSamples / SPD;
    const uint32_t cb = blockIdx.x % A.col_blocks;
    const uint32_t S0 = (blockIdx.x / A.col_blocks) * ROWS;
    const uint32_t j = cb * kInjectThreads + threadIdx.x;
    if (j >= A.nchans) return;

    // the lane's samples: row within the super-row (-3 .. 3) and channel
    int32_t q[SPD];
    uint32_t ch[SPD];
#pragma unroll
    for (uint32_t b = 0; b < SPD; ++b) {
        // e + 4 * nchans >= 0 and below 2^27: nchans <= 2^24
        const uint32_t e = SPD * j + b + 4 * A.nchans - A.m;
        q[b] = (int32_t)(e / A.nchans) - 4;
        ch[b] = e % A.nchans;
    }

    float acc[ROWS][SPD];
#pragma unroll
    for (uint32_t i = 0; i < ROWS; ++i)
#pragma unroll
        for (uint32_t b = 0; b < SPD; ++b) acc[i][b] = 0.0f;

    const int64_t t_tile = A.t_origin + (int64_t)SPD * S0;   // row 0 of super-row S0
    for (uint32_t k = 0; k < A.nspecs; ++k) {
        const rt_inject_spec sp = A.specs[k];
        const float* __restrict__ tp = A.tmpl + sp.tmpl_off;
        float a[SPD];
        int64_t u0[SPD];   // u of the lane's samples in super-row S0
#pragma unroll
        for (uint32_t b = 0; b < SPD; ++b) {
            a[b] = A.amp[sp.amp_off + ch[b]];
            u0[b] = t_tile + q[b] - (int64_t)A.delay[sp.delay_off + ch[b]];
        }
        if (sp.factor == 0.0) {
            if (sp.kind == 0) {
                const uint32_t shift = 64 - sp.log2bins;
                const uint64_t dph = sp.step * SPD;
                uint64_t ph[SPD];
#pragma unroll
                for (uint32_t b = 0; b < SPD; ++b) ph[b] = sp.phase0 + (uint64_t)u0[b] * sp.step;
#pragma unroll
                for (uint32_t i = 0; i < ROWS; ++i)
#pragma unroll
                    for (uint32_t b = 0; b < SPD; ++b) {
                        acc[i][b] = __fadd_rn(acc[i][b], __fmul_rn(a[b], tp[ph[b] >> shift]));
                        ph[b] += dph;
                    }
            } else {
#pragma unroll
                for (uint32_t i = 0; i < ROWS; ++i)
#pragma unroll
                    for (uint32_t b = 0; b < SPD; ++b) {
                        const uint64_t w = (uint64_t)u0[b] + SPD * i - (uint64_t)sp.t0;
                        const float v = w < sp.length ? __fmul_rn(a[b], tp[w]) : 0.0f;
                        acc[i][b] = __fadd_rn(acc[i][b], v);
                    }
            }
        } else {
            const uint32_t shift = 64 - sp.log2bins;
#pragma unroll
            for (uint32_t i = 0; i < ROWS; ++i)
#pragma unroll
                for (uint32_t b = 0; b < SPD; ++b) {
                    const int64_t ue = inject_time_dev(sp.factor, sp.span, u0[b] + (int64_t)(SPD * i));
                    float v;
                    if (sp.kind == 0) {
                        const uint64_t ph = sp.phase0 + (uint64_t)ue * sp.step;
                        v = __fmul_rn(a[b], tp[ph >> shift]);
                    } else {
                        const uint64_t w = (uint64_t)ue - (uint64_t)sp.t0;
                        v = w < sp.length ? __fmul_rn(a[b], tp[w]) : 0.0f;
                    }
                    acc[i][b] = __fadd_rn(acc[i][b], v);
                }
        }
    }

    // the lane's dwords: super-row S0 + i, column j
    uint32_t* __restrict__ xd = reinterpret_cast<uint32_t*>(A.x);
    if (SPD == 1) {
        float* __restrict__ xf = reinterpret_cast<float*>(A.x);
        float v[ROWS];
#pragma unroll
        for (uint32_t i = 0; i < ROWS; ++i)
            if (S0 + i < A.nsamp) v[i] = xf[(uint64_t)(S0 + i) * A.nchans + j];
#pragma unroll
        for (uint32_t i = 0; i < ROWS; ++i)
            if (S0 + i < A.nsamp) xf[(uint64_t)(S0 + i) * A.nchans + j] = __fadd_rn(v[i], acc[i][0]);
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < ROWS; ++i) {
        const uint32_t S = S0 + i;
        if (S >= A.super_rows) break;
        const uint64_t D = (uint64_t)S * A.nchans + j;
        bool ok[SPD];
        bool whole = true;
#pragma unroll
        for (uint32_t b = 0; b < SPD; ++b) {
            const int64_t r = (int64_t)SPD * S + q[b];
            ok[b] = r >= 0 && r < (int64_t)A.nsamp;
            whole = whole && ok[b];
        }
        if (whole) {
            const uint32_t w = xd[D];
            uint32_t y = 0;
#pragma unroll
            for (uint32_t b = 0; b < SPD; ++b) {
                const uint64_t t = (uint64_t)(A.t_origin + (int64_t)SPD * S + q[b]);
                const int32_t d = inject_increment_dev(acc[i][b], inject_dither_dev(t, A.nchans, ch[b], A.salt));
                y |= inject_byte<SIGNED>((w >> (8 * b)) & 0xffu, d) << (8 * b);
            }
            xd[D] = y;
        } else {
            // a dword across the block's first or last byte: its bytes inside the block, one by one
            uint8_t* xb = reinterpret_cast<uint8_t*>(A.x) + 4 * D;
#pragma unroll
            for (uint32_t b = 0; b < SPD; ++b) {
                if (!ok[b]) continue;
                const uint64_t t = (uint64_t)(A.t_origin + (int64_t)SPD * S + q[b]);
                const int32_t d = inject_increment_dev(acc[i][b], inject_dither_dev(t, A.nchans, ch[b], A.salt));
                xb[b] = (uint8_t)inject_byte<SIGNED>(xb[b], d);
            }
        }
    }
}

}  // namespace

hipError_t launch_inject(int dtype, const InjectArgs& A, uint32_t blocks, hipStream_t s)
{
    if (!blocks || !A.nspecs) return hipSuccess;
    if (dtype == RT_DEDISP_F32)
        hipLaunchKernelGGL((inject_kernel<1, false>), dim3(blocks), dim3(kInjectThreads), 0, s, A);
    else if (dtype == RT_DEDISP_I8)
        hipLaunchKernelGGL((inject_kernel<4, true>), dim3(blocks), dim3(kInjectThreads), 0, s, A);
    else
        hipLaunchKernelGGL((inject_kernel<4, false>), dim3(blocks), dim3(kInjectThreads), 0, s, A);
    return hipGetLastError();
}

}  // namespace rt
