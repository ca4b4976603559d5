// Launch wrappers of the HIP kernels (host-callable, stream-ordered, no sync).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "dered_host.hpp"
#include "fold_host.hpp"
#include "harmonic.hpp"
#include "inject_host.hpp"
#include "refine_host.hpp"
#include "resample_host.hpp"
#include "riptide_amd.h"

namespace rt {

// ladder_kernels.hip
hipError_t launch_downsample_ladder(const float* x, uint64_t n_in, uint64_t x_stride,
                                    const DsRung* d_rungs, uint32_t num_rungs, uint32_t total_blocks,
                                    float* out, uint64_t out_stride, uint32_t batch, hipStream_t s);
// all rungs of a periodogram from one read of the series; margin: samples
// staged past each span, ds_fused_margin(rungs) of common.hpp (every rung: ceil(f) + 2 <= margin <= kDsFusedMargin)
hipError_t launch_downsample_fused(const float* x, uint64_t n_in, uint64_t x_stride, const DsRung* d_rungs,
                                   uint32_t num_rungs, uint32_t margin, float* out, uint64_t out_stride,
                                   uint32_t batch, hipStream_t s);

// ffa_kernels.hip (the cone kernel's parts: cone_unit.hpp, cone_merge.hpp, cone_snr.hpp)
// smax: merge_slots() bucket covering every transform of the launch
hipError_t launch_cone(const ConeArgs& args, uint32_t smax, bool wide_snr, uint32_t snr,
                       hipStream_t s);   // grid (num_items, batch); wide_snr, snr (kSnrNone / kSnrRows / kSnrSeg): the Launch's
hipError_t launch_ffa_level(const float* in, float* out, const uint2* d_nodes, uint32_t num_nodes,
                            uint32_t rows, uint32_t p, hipStream_t s);

// peaks_kernels.hip
constexpr int kMaxSegmentPoints = 32768;  // rows of one peak-detection segment sorted in LDS (128 KiB)
constexpr int kMaxSegmentRanks = 8;       // order statistics per segment (host ranks array)
hipError_t launch_segment_order_stats(const float* snrs, uint64_t snr_stride, uint32_t batch, uint32_t W,
                                      uint32_t nseg, uint32_t per_seg, const uint32_t* ranks, uint32_t nranks,
                                      float* out, hipStream_t s);
hipError_t launch_threshold_select(const float* snrs, uint64_t snr_stride, uint32_t batch, uint32_t L, uint32_t W,
                                   const double* logf, const double* coeffs, uint32_t ncoef, double smin,
                                   uint32_t* counts, uint32_t* idx, uint32_t cap, hipStream_t s);
// clustered peaks of every (trial, width): chunk = peak_chunk_rows(), workspace
// = peak_workspace_bytes() bytes (peaks_host.hpp), 8-byte aligned
hipError_t launch_find_peaks(const float* snrs, uint64_t snr_stride, uint32_t batch, uint32_t L, uint32_t W,
                             const double* logf, const double* freqs, const double* coeffs, uint32_t ncoef,
                             double smin, double r, uint32_t* counts, uint32_t* rows, float* out, uint32_t cap,
                             uint32_t chunk, void* workspace, hipStream_t s);

hipError_t launch_convert_samples(const void* raw, uint64_t n, int is_signed, float* out, hipStream_t s);

// aux_kernels.hip
hipError_t launch_snr_rows(const float* x, uint64_t rows, uint32_t cols, const uint32_t* d_widths,
                           uint32_t nw, float stdnoise, float* cps_scratch, float* out, hipStream_t s);
hipError_t launch_running_median(const float* x, uint64_t n, uint32_t width, float* out, uint64_t x_stride,
                                 uint64_t out_stride, uint32_t batch, hipStream_t s);
hipError_t launch_scrunch(const float* x, uint64_t n_out, uint32_t factor, float* out, uint64_t x_stride,
                          uint64_t out_stride, uint32_t batch, hipStream_t s);
hipError_t launch_deredden_subtract(const float* x, uint64_t n, const float* rmed_lo, uint64_t n_lo,
                                    uint32_t factor, float* out, uint64_t x_stride, uint64_t lo_stride,
                                    uint64_t out_stride, uint32_t batch, hipStream_t s, double* slopes = nullptr);
// dereddening + normalisation with the normalisation's statistics summed by
// the dereddening kernel (no read pass of their own).  Applies when
// dered_norm_fusable(); partials: batch * 2 * dered_norm_blocks(n) doubles
// (dered_host.hpp),
// stats: 2 * batch doubles.
bool dered_norm_fusable(const float* x, uint64_t n, uint64_t n_lo, uint32_t factor, const float* out,
                        uint64_t x_stride, uint64_t out_stride);
hipError_t launch_deredden_normalise(const float* x, uint64_t n, const float* rmed_lo, uint64_t n_lo,
                                     uint32_t factor, float* out, uint64_t x_stride, uint64_t lo_stride,
                                     uint64_t out_stride, uint32_t batch, hipStream_t s, double* slopes,
                                     double* partials, double* stats);
hipError_t launch_interp(uint64_t n, const float* rmed_lo, uint64_t n_lo, uint32_t factor, double* out,
                         hipStream_t s);
hipError_t launch_normalise(const float* x, uint64_t n, float* out, double* d_partials, uint32_t nblocks,
                            uint64_t x_stride, uint64_t out_stride, uint32_t batch, hipStream_t s);
hipError_t launch_rollback(const float* x, uint64_t n, uint64_t shift, const float* y, float* out, hipStream_t s);
hipError_t launch_circular_prefix_sum(const float* x, uint64_t n, uint64_t nsum, float* out, hipStream_t s);

// fold_kernels.hip
// the candidate descriptor FoldCand and its modes: fold_host.hpp
hipError_t launch_fold_rows(const float* data, uint64_t n_in, const FoldCand* d_cands, uint32_t num_cands,
                            uint32_t total_blocks, float* out, float* rows_ws, hipStream_t s);
hipError_t launch_fold_subints(const FoldCand* d_cands, uint32_t num_cands, uint32_t total_blocks, float* out,
                               const float* rows_ws, hipStream_t s);

// refine_kernels.hip
// the candidate descriptor RefineCand and the plan's block counts and LDS
// bytes: refine_host.hpp.  Stage A (y of every candidate into d_y), then stage
// B (S/N, and the profiles unless d_profiles is null).
hipError_t launch_refine(const float* d_cubes, const int32_t* d_shifts, const uint32_t* d_widths,
                         const RefineCand* d_cands, uint32_t num_cands, uint32_t blocks_a, uint32_t blocks_b,
                         uint32_t lds_a, uint32_t lds_b, float* d_y, float* d_snr, float* d_profiles, hipStream_t s);

// dedisp_kernels.hip (the sample type codes and the shared checks: dedisp_types.hpp)
// bytes of one channel-major row of the transposed block (dtype: the
// RT_DEDISP_* code of riptide_amd.h), a multiple of 16: bytes for 8-bit and
// 1/2/4-bit data, floats for float and 16-bit data
uint64_t dedisp_pitch_bytes(int dtype, uint64_t nsamp_blk);
// out[d * out_stride + t] for t < nsamp_blk - max_delay; ws: nchans rows of
// dedisp_pitch_bytes, 16-byte aligned.  The caller has checked the shape
// (rt_dedisperse_device).
// flags: 0 or RT_DEDISP_ZERO_DM (the zero-DM filter: m = the rows' means over
// the unmasked channels, float rows of x - m, the float sum for every dtype).
// bytes of ws for these flags: the rows, with RT_DEDISP_ZERO_DM float rows plus
// one more pitch for m [nsamp_blk]
uint64_t dedisp_workspace_bytes(int dtype, uint64_t nsamp_blk, uint64_t nchans, uint32_t flags);
// A block mask in device memory (rt_block_mask of riptide_amd.h, checked by
// the caller: every row of the block lies in a block of cells): sample (t, c)
// is read as fill[c] where cells[(t_origin + t) / block_len, c] != 0; fill is
// one value per channel in the sample's own type.
struct DedispCells {
    const uint8_t* cells;   // [nblocks, nchans]
    const void* fill;       // [nchans]
    uint64_t t_origin;
    uint64_t block_len;
};
// d_bands: nullptr, or uint32 [nbands][2] channel ranges [lo, hi) in device
// memory (clamped to nchans as they are read): out[(d * nbands + b) *
// out_stride + t] is then the sum over band b alone; nbands <= 65535
// (RT_DEDISP_MAX_BANDS), a grid layer per band.
// bm: nullptr (the plain kernels), or a block mask (their DdCells forms).
hipError_t launch_dedisperse(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                             const int32_t* d_delays, const uint8_t* d_mask, uint32_t ndm, uint32_t max_delay,
                             float* out, uint64_t out_stride, void* ws, uint32_t flags, hipStream_t s,
                             const uint32_t* d_bands = nullptr, uint32_t nbands = 0,
                             const DedispCells* bm = nullptr);
// launch_dedisperse's first step alone: the block (with bm: x') to the
// channel-major rows of ws -- float32 rows when dedisp_float_rows(dtype, flags)
// (under RT_DEDISP_ZERO_DM x - m, m behind the rows), 8-bit rows otherwise
// (int8 biased by 128, 1/2/4-bit unpacked); the padding of a row, elements
// [nsamp_blk, pitch), is written as zero
hipError_t launch_dedisp_rows(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                              const uint8_t* d_mask, void* ws, uint32_t flags, hipStream_t s,
                              const DedispCells* bm = nullptr);
// dedisp_workspace_bytes for a step table: those rows, then for min_factor, the
// smallest downsamp > 1 of the call (0: none), one float32 area of nchans rows
// of nsamp_blk / min_factor samples at dedisp_pitch_bytes(RT_DEDISP_F32, .),
// which every decimated step reuses in stream order
uint64_t dedisp_steps_workspace_bytes(int dtype, uint64_t nsamp_blk, uint64_t nchans, uint32_t flags,
                                      uint32_t min_factor);
// Every step of a table (host memory, checked by the caller: dedisp_check_steps)
// from one launch_dedisp_rows: a step of downsamp 1 is launch_dedisperse's sum;
// any other decimates the rows into the float32 area (dedisp_decimate_kernel,
// the padding of its pitch written as zero) and runs the float32 sum over it.
// Step k writes out[out_off + d * out_stride + out_offset + u], u < nsamp_blk /
// downsamp - max_delay, with the delays from d_delays + delays_off.
hipError_t launch_dedisperse_steps(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                                   const int32_t* d_delays, const uint8_t* d_mask, const rt_dedisp_step* steps,
                                   size_t nsteps, float* out, void* ws, uint32_t flags, hipStream_t s,
                                   const DedispCells* bm = nullptr);
// m[t] = (float32)(sum over unmasked c of block[t, c] / their number), t < nsamp_blk
hipError_t launch_zero_dm_mean(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans,
                               const uint8_t* d_mask, float* m, hipStream_t s, const DedispCells* bm = nullptr);
// acc [2, nchans] float64 += the block's per-channel sums and sums of squares;
// ws: chanstats_workspace_bytes of per-chunk partial sums
uint64_t chanstats_workspace_bytes(uint64_t nsamp_blk, uint64_t nchans);
hipError_t launch_channel_stats(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans, double* acc,
                                void* ws, hipStream_t s);
// stats [ceil(nsamp_blk / block_len), 2, nchans] float64 = those sums per block
// of block_len rows (written); ws: blockstats_workspace_bytes (none up to 2048
// rows a block).  blockstats_chunks: the workgroups along x, below 2^31
uint64_t blockstats_chunks(uint64_t nsamp_blk, uint64_t block_len);
uint64_t blockstats_workspace_bytes(uint64_t nsamp_blk, uint64_t nchans, uint64_t block_len);
hipError_t launch_block_stats(const void* block, int dtype, uint32_t nsamp_blk, uint32_t nchans, uint32_t block_len,
                              double* stats, void* ws, hipStream_t s);

// cutout_kernels.hip (the tile, the staging rule and the checks: cutout_host.hpp)
// ws: the rows launch_dedisp_rows left for this dtype and these flags.  Job i
// of d_jobs (device memory, checked by the caller: cutout_check_jobs) writes
// its nbins floats from out + out_off; max_tiles = ceil(the largest nbins /
// kCutoutTile) <= kCutoutMaxTiles, njobs >= 1.
hipError_t launch_pulse_cutouts(const void* ws, int dtype, uint32_t flags, uint32_t nsamp_blk, uint32_t nchans,
                                const int32_t* d_delays, uint32_t ndelay_rows, uint32_t max_delay,
                                const uint8_t* d_mask, const rt_cutout_spec* d_jobs, uint32_t njobs,
                                uint32_t max_tiles, float* out, hipStream_t s);

// resample_kernels.hip
// out[r, j] = x[T.src[r], resample_index(T.factor[r], j, N)] for r < rows <=
// kResampleLaunchRows, j < N; the caller has checked the table
// (resample_check_args of resample_host.hpp)
hipError_t launch_resample(const float* x, uint64_t ldx, uint32_t N, const ResampleRows& T, uint32_t rows,
                           float* out, uint64_t ldo, hipStream_t s);

// inject_kernels.hip
// the specification of inject_host.hpp in place on the block A.x + A.m; A and
// blocks are inject_shape's, the table has passed inject_check_table
hipError_t launch_inject(int dtype, const InjectArgs& A, uint32_t blocks, hipStream_t s);

// harmonic_kernels.hip
// One tile of the harmonic pair matrix: rows [i0, i0 + rows) of the n ranked
// clusters, wpr = ceil(n / 64) 64-bit words per row, bit j of row i =
// htest(i, j) for j > i.  *near_count (zeroed by the caller) counts the pairs
// the host must decide; the first near_cap of them are listed as (i, j).
hipError_t launch_harmonic_pairs(const double* freq, const double* snr, const double* ducy, const double* dm,
                                 uint32_t n, uint32_t i0, uint32_t rows, uint32_t wpr, const HParams& P,
                                 uint64_t* words, uint2* near_list, uint32_t near_cap, uint32_t* near_count,
                                 hipStream_t s);
hipError_t launch_harmonic_diag(const double* freq, const double* snr, const double* ducy, const double* dm,
                                const int32_t* pi, const int32_t* pj, uint64_t npairs, const HParams& P, int64_t* num,
                                int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance,
                                hipStream_t s);

}  // namespace rt
