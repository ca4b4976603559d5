// Pulse cutouts for MI355X (gfx950): dedispersed, time-decimated windows of a
// resident block, one per job (the specification: rt_pulse_cutouts_host,
// cutout_host.cpp; the definition: riptide_amd.h)
//   out[out_off + n] = sum over unmasked c in [band_lo, band_hi) of
//                      sum over j < f of x'[start + n f + j + delay[row][c], c]
// read from the channel-major rows that launch_dedisp_rows (dedisp_kernels.hip)
// leaves in the dedispersion workspace: 8-bit rows (int8 biased by 128) or
// float32 rows.
//
//   pulse_cutout_kernel<T>  one workgroup = one job x one tile of kCutoutTile
//                           bins, a lane per bin, so the lanes of a wave walk
//                           along a channel's row.  A bin is owned by one lane
//                           from its first channel to its last: the float sum
//                           is the sequential one of the specification.  Per
//                           step of kCutoutChans channels every wave stages
//                           the spans of two channels in LDS with coalesced
//                           dword loads (cutout_host.hpp has the rule: a span
//                           longer than kCutoutSpanDwords is read from the row
//                           directly), then every lane adds its f samples of
//                           each channel.  8-bit samples are summed a dword at
//                           a time (bytes outside the bin masked off, four
//                           bytes per v_sad_u8); floats one rounded addition
//                           per sample, j ascending.
//
// The two paths differ in where a dword comes from and in nothing else, so
// they give the same bits.  No load leaves the workspace: a job's band edges,
// its delay row and every delay are clamped as they are read, and a lane's
// samples are clamped to [0, nsamp_blk) before anything is addressed -- what
// lies outside is skipped, as the specification skips it, and for int8 data
// the bias is taken off once per sample that was added.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "cutout_host.hpp"
#include "kernels.hpp"

namespace rt {

namespace {

constexpr uint32_t kCtThreads = kCutoutTile;
constexpr uint32_t kCtWaves = kCtThreads / 64;
constexpr uint32_t kCtSkip = 0xFFFFFFFFu;     // channel masked, past the band, or its span outside the block
constexpr uint32_t kCtDirect = 0xFFFFFFFEu;   // span too long to stage: read from the workspace row

// the sum of the bytes [b, e) of a row, b < e, fetch(w) its dword w
template <class Fetch>
__device__ inline uint32_t ct_sum_bytes(uint32_t b, uint32_t e, Fetch fetch)
{
    uint32_t acc = 0;
    const uint32_t w1 = (e - 1) >> 2;
    for (uint32_t w = b >> 2; w <= w1; ++w) {
        const uint32_t lo = max(b, 4 * w) - 4 * w;          // bytes [lo, hi) of this dword, hi - lo >= 1
        const uint32_t hi = min(e, 4 * w + 4) - 4 * w;
        const uint32_t keep = (0xFFFFFFFFu >> (8 * (4 - hi))) & (0xFFFFFFFFu << (8 * lo));
        acc = __builtin_amdgcn_sad_u8(fetch(w) & keep, 0u, acc);
    }
    return acc;
}

// T = uint8_t (bias 128 for int8 data, else 0) or float; pitch in elements.
template <class T>
__global__ __launch_bounds__(kCtThreads) void pulse_cutout_kernel(
    const T* __restrict__ ws, uint64_t pitch, uint32_t nsamp, uint32_t nchans, const int32_t* __restrict__ delays,
    uint32_t ndelay_rows, uint32_t max_delay, const uint8_t* __restrict__ mask,
    const rt_cutout_spec* __restrict__ jobs, float* __restrict__ out, int32_t bias)
{
    constexpr bool kBytes = sizeof(T) == 1;
    constexpr uint32_t kE = 4 / sizeof(T);   // elements per dword
    __shared__ uint32_t span[kCutoutChans][kCutoutSpanDwords];
    __shared__ uint32_t sbase[kCutoutChans];   // first element staged, or kCtSkip / kCtDirect
    __shared__ int32_t sdel[kCutoutChans];

    const rt_cutout_spec job = jobs[blockIdx.x];
    const uint32_t t0 = blockIdx.y * kCutoutTile;
    if (t0 >= job.nbins) return;   // uniform: before any barrier
    const uint32_t nb = min(kCutoutTile, job.nbins - t0);
    const uint32_t f = job.factor;
    const uint32_t c_hi = min(job.band_hi, nchans), c_lo = min(job.band_lo, c_hi);
    const int32_t* del = delays + (uint64_t)min(job.delay_row, ndelay_rows - 1) * nchans;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // first sample of the tile, and of this lane's bin, at delay 0: |start| <= 2^40 and nbins * f < 2^31
    const int64_t tile_first = job.start + (int64_t)t0 * f;
    const int64_t bin_first = tile_first + (int64_t)tid * f;
    const bool live = tid < nb;

    using Acc = typename std::conditional<kBytes, uint32_t, float>::type;
    Acc acc = 0;
    uint32_t count = 0;   // 8-bit: samples added, which the bias correction multiplies

    for (uint32_t c0 = c_lo; c0 < c_hi; c0 += kCutoutChans) {
        __syncthreads();   // the previous step's spans are consumed
        for (uint32_t cc = wave; cc < kCutoutChans; cc += kCtWaves) {
            const uint32_t c = c0 + cc;
            uint32_t base = kCtSkip;
            int32_t d = 0;
            if (c < c_hi && !(mask && mask[c])) {
                d = min(max(del[c], 0), (int32_t)max_delay);
                // the tile's span of this channel, clamped to the block
                const int64_t a = tile_first + d;
                const int64_t lo = max(a, (int64_t)0), hi = min(a + (int64_t)nb * f, (int64_t)nsamp);
                if (lo < hi) {
                    const CutoutSpan sp = cutout_span(sizeof(T), (uint32_t)lo, (uint32_t)hi);
                    if (sp.direct) {
                        base = kCtDirect;
                    } else {
                        // dwords [first / kE, first / kE + ndw): the last one holds element hi - 1 < nsamp <= pitch
                        const uint32_t* row = reinterpret_cast<const uint32_t*>(ws + (uint64_t)c * pitch);
                        const uint32_t w0 = sp.first / kE;
                        for (uint32_t i = lane; i < sp.ndw; i += 64) span[cc][i] = row[w0 + i];
                        base = sp.first;
                    }
                }
            }
            if (lane == 0) {
                sbase[cc] = base;
                sdel[cc] = d;
            }
        }
        __syncthreads();

        for (uint32_t cc = 0; cc < kCutoutChans; ++cc) {
            const uint32_t base = __builtin_amdgcn_readfirstlane(sbase[cc]);
            if (base == kCtSkip) continue;
            const int32_t d = __builtin_amdgcn_readfirstlane(sdel[cc]);
            // this lane's samples of the channel, clamped to the block
            const int64_t a = bin_first + d;
            const int64_t lo64 = max(a, (int64_t)0), hi64 = min(a + (int64_t)f, (int64_t)nsamp);
            if (!live || lo64 >= hi64) continue;
            const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)hi64;
            const T* row = ws + (uint64_t)(c0 + cc) * pitch;
            if constexpr (kBytes) {
                const uint32_t* row32 = reinterpret_cast<const uint32_t*>(row);
                if (base == kCtDirect) {
                    acc += ct_sum_bytes(lo, hi, [&](uint32_t w) { return row32[w]; });
                } else {
                    const uint32_t w0 = base >> 2;
                    acc += ct_sum_bytes(lo, hi, [&](uint32_t w) { return span[cc][w - w0]; });
                }
                count += hi - lo;
            } else {
                if (base == kCtDirect) {
                    for (uint32_t e = lo; e < hi; ++e) acc = __fadd_rn(acc, row[e]);
                } else {
                    for (uint32_t e = lo; e < hi; ++e) acc = __fadd_rn(acc, __uint_as_float(span[cc][e - base]));
                }
            }
        }
    }

    if (!live) return;
    float* o = out + job.out_off + t0 + tid;
    if constexpr (kBytes) *o = (float)((int32_t)acc - bias * (int32_t)count);
    else *o = acc;
}

}  // namespace

hipError_t launch_pulse_cutouts(const void* ws, int dtype, uint32_t flags, uint32_t nsamp_blk, uint32_t nchans,
                                const int32_t* d_delays, uint32_t ndelay_rows, uint32_t max_delay,
                                const uint8_t* d_mask, const rt_cutout_spec* d_jobs, uint32_t njobs,
                                uint32_t max_tiles, float* out, hipStream_t s)
{
    const bool float_rows = dedisp_float_rows(dtype, flags);
    const uint64_t pitch_bytes = dedisp_pitch_bytes(float_rows ? RT_DEDISP_F32 : dtype, nsamp_blk);
    const dim3 grid(njobs, max_tiles);
    if (float_rows)
        hipLaunchKernelGGL(pulse_cutout_kernel<float>, grid, dim3(kCtThreads), 0, s, (const float*)ws, pitch_bytes / 4,
                           nsamp_blk, nchans, d_delays, ndelay_rows, max_delay, d_mask, d_jobs, out, 0);
    else
        hipLaunchKernelGGL(pulse_cutout_kernel<uint8_t>, grid, dim3(kCtThreads), 0, s, (const uint8_t*)ws, pitch_bytes,
                           nsamp_blk, nchans, d_delays, ndelay_rows, max_delay, d_mask, d_jobs, out,
                           dtype == RT_DEDISP_I8 ? 128 : 0);
    return hipGetLastError();
}

}  // namespace rt
