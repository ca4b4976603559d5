/*
 * riptide_amd.h -- C ABI of the MI355X-native FFA periodogram engine.
 *
 * This is the drop-in boundary for riptide's native module `riptide.libcpp`
 * (pybind11, /root/reference/riptide/cpp/python_bindings.cpp:213-267).  Each
 * host-buffer entry point below replaces one binding of that module, with the
 * same argument meaning, output shape/dtype and error text; the Python shim
 * riptide_amd/libcpp.py (or the ctypes stub in INTEGRATION.md) maps them onto
 * the reference's function names.  All compute runs in HIP kernels on the
 * current device; there is no CPU compute path.
 *
 * Conventions
 *  - Return value: RT_OK (0) on success; RT_EINVAL for the cases where the
 *    reference throws std::invalid_argument / std::domain_error (Python
 *    ValueError); RT_EHIP for a HIP runtime failure; RT_EINTERNAL otherwise.
 *    rt_last_error() returns the message of the calling thread's last failure
 *    (the reference's exception text for RT_EINVAL).
 *  - "host" pointers are ordinary CPU memory (numpy buffers); "device"
 *    pointers are HIP device memory; `stream` is a hipStream_t (NULL = the
 *    library's own stream).  Host-buffer calls are synchronous.
 *  - Widths are uint64 (size_t in the reference).
 */
#ifndef RIPTIDE_AMD_H
#define RIPTIDE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_EINVAL 1
#define RT_EHIP 2
#define RT_EINTERNAL 3

const char* rt_last_error(void);
/* Version string of the engine and the gfx target it was built for. */
const char* rt_version(void);
/* Select the HIP device used by subsequent host-buffer calls of this thread. */
int rt_set_device(int device);

/* ---------------- host-buffer drop-ins for riptide.libcpp ----------------- */

/* python_bindings.cpp:32-40  rollback(x, shift): out = roll(x, -shift) */
int rt_rollback(const float* x, size_t size, size_t shift, float* out);

/* python_bindings.cpp:43-58  fused_rollback_add(x, y, shift): out = x + roll(y, -shift) */
int rt_fused_rollback_add(const float* x, const float* y, size_t size, size_t shift, float* out);

/* python_bindings.cpp:61-69  circular_prefix_sum(x, nsum): out has nsum elements */
int rt_circular_prefix_sum(const float* x, size_t size, size_t nsum, float* out);

/* python_bindings.cpp:72-84  ffa2(data[rows, cols]) -> out[rows, cols] */
int rt_ffa2(const float* in, size_t rows, size_t cols, float* out);

/* python_bindings.cpp:87-106  benchmark_ffa2(rows, cols, loops) -> seconds per loop
 * (device-resident zero input, HIP-event timed) */
int rt_benchmark_ffa2(size_t rows, size_t cols, size_t loops, double* seconds);

/* python_bindings.cpp:109-126  snr1(data[size], widths, stdnoise) -> out[num_widths] */
int rt_snr1(const float* x, size_t size, const uint64_t* widths, size_t num_widths, float stdnoise, float* out);

/* python_bindings.cpp:129-148  snr2(data[rows, cols], widths, stdnoise) -> out[rows, num_widths] */
int rt_snr2(const float* x, size_t rows, size_t cols, const uint64_t* widths, size_t num_widths,
            float stdnoise, float* out);

/* downsample.hpp:21-24  floor(size / f) */
size_t rt_downsampled_size(size_t size, double f);

/* python_bindings.cpp:151-165  downsample(data, factor) -> out[rt_downsampled_size(size, factor)] */
int rt_downsample(const float* x, size_t size, double factor, float* out);
/* Row-wise downsampling of a rows x size array by the same factor: rows x
 * downsampled_size(size, f) floats (the batched form folding.py's
 * downsample_vertical needs; same arithmetic as rt_downsample). */
int rt_downsample_rows(const float* x, size_t rows, size_t size, double f, float* out);

/* periodogram.hpp:63-109  number of trial periods (validates arguments) */
int rt_periodogram_length(size_t size, double tsamp, double period_min, double period_max,
                          size_t bins_min, size_t bins_max, size_t* length);

/* python_bindings.cpp:168-197  periodogram(data, tsamp, widths, period_min, period_max,
 * bins_min, bins_max) -> periods[L] (f64), foldbins[L] (u32), snrs[L, num_widths] (f32) */
int rt_periodogram(const float* data, size_t size, double tsamp, const uint64_t* widths, size_t num_widths,
                   double period_min, double period_max, size_t bins_min, size_t bins_max,
                   double* periods, uint32_t* foldbins, float* snrs);

/* python_bindings.cpp:200-210  running_median(data, width) -> out[size] */
int rt_running_median(const float* x, size_t size, size_t width, float* out);

/* running_medians.py:49-83 fast_running_median(data, width_samples, min_points) for a
 * scrunch factor > 1: float32 block means, exact running median of width
 * min_points, np.interp back to full resolution -> out[size] (float64).  A
 * scrunch factor of 1 is rt_running_median (the reference returns float32 then). */
int rt_fast_running_median(const float* x, size_t size, size_t width_samples, size_t min_points, double* out);

/* time_series.py:93-122 + :66-90 (TimeSeries.deredden(width_samples, minpts) then
 * .normalise()), one series; either stage may be skipped. width_samples is
 * int(round(rmed_width / tsamp)) computed by the caller (Python round). */
int rt_deredden_normalise(const float* x, size_t size, size_t width_samples, size_t min_points,
                          int deredden, int normalise, float* out);

/* periodogram.hpp:190-194  trial-period grid only (host computation, no device) */
int rt_periodogram_grid(size_t size, double tsamp, double period_min, double period_max, size_t bins_min,
                        size_t bins_max, double* periods, uint32_t* foldbins);

/* Host-only: build the FFA pass schedule for a periodogram and verify its
 * invariants (tiles inside nodes, LDS budget, final pass covers every row). */
int rt_schedule_check(size_t size, double tsamp, size_t num_widths, double period_min, double period_max,
                      size_t bins_min, size_t bins_max, uint64_t* transforms, uint64_t* items,
                      uint64_t* launches, double* alg_bytes_per_trial, double* moved_bytes_per_trial,
                      uint64_t* cells_per_trial);

/* Host-only: the pass schedule rt_plan_create builds for these parameters and
 * boxcar widths (built and validated as in rt_schedule_check), with its final
 * launches -- the ones that end in the fused S/N -- counted by S/N kind: the
 * row-group form and the segmented form (rows of 240-264 bins, widths <= 9,
 * <= 64 rows per unit) run separate kernel instances, so no launch mixes them.
 * *launches = all cone launches; bins_kinds[b] for b < bins_cap gets bit 0 if
 * a final unit of b phase bins runs in a row-group launch, bit 1 if one runs
 * in a segmented launch.  Every output pointer may be NULL. */
int rt_schedule_final_kinds(size_t size, double tsamp, const uint64_t* widths, size_t num_widths, double period_min,
                            double period_max, size_t bins_min, size_t bins_max, uint64_t* launches,
                            uint64_t* rows_launches, uint64_t* seg_launches, uint8_t* bins_kinds, size_t bins_cap);

/* Host-only, no device: the work units of the pass schedule
 * rt_schedule_check builds for these parameters, in dispatch order (the
 * workgroups of a launch start in this order), launch after launch.  A unit
 * of a pass-0 launch (src_leaves = 1) reads the floats [node_start * bins,
 * (node_start + node_size) * bins) of its rung's downsampled series.
 * Writes min(*count, cap) records (items may be NULL when cap == 0); *count
 * may be NULL. */
typedef struct rt_schedule_item {
    uint32_t launch;      /* index of the unit's launch */
    uint32_t pass;        /* the launch's pass within its transform group */
    uint32_t slots;       /* the launch's kernel variant (merge slot width) */
    uint32_t snr_kind;    /* 0 merge-only, 1 / 2 final with the row-group / segmented S/N */
    uint32_t xform;       /* transform index */
    uint32_t rung;        /* the transform's ladder rung */
    uint32_t bins;        /* the transform's phase bins */
    uint32_t node_start, node_size;   /* target node, rows of the transform */
    uint32_t s0, s1;      /* output rows [s0, s1) within the node */
    uint32_t levels;      /* merge levels the unit evaluates */
    uint32_t src_leaves;  /* 1: the unit fills from the rung leaf buffer */
    uint32_t tile;        /* 0: a whole node in LDS, 1: a tile of a node's upper levels */
} rt_schedule_item;
int rt_schedule_items(size_t size, double tsamp, size_t num_widths, double period_min, double period_max,
                      size_t bins_min, size_t bins_max, rt_schedule_item* items, size_t cap, uint64_t* count);

/* Host-only: the downsampling-ladder kernel a periodogram plan of these
 * parameters runs (periodogram.hpp:162-168 restated per rung): *fused = 1
 * for the one-read fused ladder (32-bit sample indices: series below 2^29
 * samples, every rung's window inside its staging margin), 2 for the fused
 * ladder over the rungs inside the margin plus the per-rung kernel for the
 * wider ones, 0 for the per-rung kernel alone (64-bit indices); *rungs =
 * rungs that feed a transform.  Either pointer may be NULL. */
int rt_ladder_check(size_t size, double tsamp, double period_min, double period_max, size_t bins_min,
                    size_t bins_max, int* fused, uint64_t* rungs);

/* Host-only, no device: where a plan of these parameters puts its ladder.
 * One record per rung that feeds a transform, in ladder order (the rungs
 * rt_ladder_check counts): a trial's leaf buffer holds rung i as n floats at
 * float offset leaf_off (16-byte aligned slots; the floats between a rung's
 * end and the next slot are never written), trial b's buffer at b *
 * leaf_floats floats from the start of the workspace.  fused = 1: the fused
 * ladder kernel writes the rung, 0: the per-rung kernel does.
 * Writes min(*count, cap) records (rungs may be NULL when cap == 0); *mode is
 * rt_ladder_check's *fused; *margin the samples the fused kernel stages past
 * each span (ceil(f) + 2 of its widest rung, rounded up to 64, at most 512;
 * 0 when it does not run).  Every output pointer may be NULL.
 * This is the layout rt_plan_create builds, from the same code, with one
 * exception: the environment variable RIPTIDE_AMD_PER_RUNG_LADDER, which
 * only rt_plan_create honours, sends every rung to the per-rung kernel
 * (mode 0) and leaves f, n, leaf_off and leaf_floats as reported here. */
typedef struct rt_ladder_rung {
    double   f;          /* downsampling factor (1: the series itself) */
    uint64_t n;          /* samples of the rung, rt_downsampled_size(size, f) */
    uint64_t leaf_off;   /* float offset in a trial's leaf buffer */
    uint32_t fused;
    uint32_t reserved;
} rt_ladder_rung;
int rt_ladder_layout(size_t size, double tsamp, double period_min, double period_max, size_t bins_min,
                     size_t bins_max, rt_ladder_rung* rungs, size_t cap, uint64_t* count, uint64_t* leaf_floats,
                     int* mode, uint32_t* margin);

/* The pass schedule rt_ffa2 runs for one rows x cols transform, built and
 * validated on the host only (validate_exec_plan: tiles, LDS budgets, unit
 * blobs, DMA segments, row slots); no device needed.  *launches may be NULL. */
int rt_ffa_schedule_check(size_t rows, size_t cols, uint64_t* launches);

/* ------------------ device-resident batched hot path ---------------------- */

typedef struct rt_plan rt_plan;

/* Build the periodogram plan (ladder, grid, pass schedule) once per
 * (size, tsamp, widths, period range, bins range).  Validates like
 * periodogram.hpp:25-40 and snr.hpp:21-31 (widths < bins_min). */
int rt_plan_create(size_t size, double tsamp, const uint64_t* widths, size_t num_widths,
                   double period_min, double period_max, size_t bins_min, size_t bins_max,
                   rt_plan** plan);
void rt_plan_destroy(rt_plan* plan);
/* L (number of trial periods) and W (number of widths). */
int rt_plan_shape(const rt_plan* plan, size_t* length, size_t* num_widths);
/* Host copy of the trial-period grid (bit-exact with the reference). */
int rt_plan_grid(const rt_plan* plan, double* periods, uint32_t* foldbins);
/* Device workspace bytes needed to process `batch` trials per call. */
int rt_plan_workspace_bytes(const rt_plan* plan, size_t batch, size_t* bytes);

/* Periodogram S/N of `batch` series resident in device memory.
 *   d_data  : batch x size floats, series b at d_data + b * data_stride
 *   d_snrs  : batch x (L * W) floats, trial b at d_snrs + b * snr_stride
 * The series must already be dereddened/normalised as the caller wants
 * (rt_deredden_normalise_device).  Stream-ordered, no host synchronisation. */
int rt_periodogram_device(const rt_plan* plan, const float* d_data, size_t batch, size_t data_stride,
                          float* d_snrs, size_t snr_stride, void* d_workspace, size_t workspace_bytes,
                          void* stream);
/* rt_periodogram_device in two stream-ordered halves, so a pipelined caller
 * can run batch k + 1's downsampling ladder (periodogram.hpp:162-168) on one
 * stream while batch k's FFA passes + S/N run on another: the ladder fills
 * the workspace's leaf buffer, the passes read it (same workspace, same
 * batch).  ladder then passes == rt_periodogram_device. */
int rt_periodogram_ladder_device(const rt_plan* plan, const float* d_data, size_t batch, size_t data_stride,
                                 void* d_workspace, size_t workspace_bytes, void* stream);
int rt_periodogram_passes_device(const rt_plan* plan, size_t batch, float* d_snrs, size_t snr_stride,
                                 void* d_workspace, size_t workspace_bytes, void* stream);

/* Device error flag of a plan: the cone kernel refuses (and leaves unwritten)
 * any work unit that breaks its LDS / register budget and raises the plan's
 * sticky flag.  Reads it on `stream` (synchronising that stream), clears it,
 * and returns RT_EINTERNAL if it was set.  The reference has no such state
 * (a CPU transform cannot run out of LDS); the host entry point
 * rt_periodogram checks it itself, as riptide::periodogram
 * (periodogram.hpp:117-201) would raise. */
int rt_plan_check(const rt_plan* plan, void* stream);

/* Device workspace bytes for rt_deredden_normalise_device. */
int rt_deredden_workspace_bytes(size_t size, size_t width_samples, size_t min_points, size_t batch,
                                size_t* bytes);
/* Batched dereddening + normalisation in device memory (d_out may equal d_in
 * only when deredden == 0). */
int rt_deredden_normalise_device(const float* d_in, size_t size, size_t batch, size_t in_stride,
                                 size_t width_samples, size_t min_points, int deredden, int normalise,
                                 float* d_out, size_t out_stride, void* d_workspace, size_t workspace_bytes,
                                 void* stream);

/* Host-only, no device: the kernel form each stage of
 * rt_deredden_normalise_device takes for rows of `size` samples whose first
 * row starts in_align / out_align bytes past a 16-byte boundary (the device
 * addresses mod 16), with rows in_stride / out_stride floats apart.  A stage
 * the call does not run reports 0.  The environment switches
 * (RIPTIDE_AMD_INTERP_PER_SAMPLE, RIPTIDE_AMD_NORM_UNFUSED,
 * RIPTIDE_AMD_NORM_SCALAR, RIPTIDE_AMD_RMED_COUNTING), which the launchers
 * read per call, are not reflected.  Validates like the device call. */
enum {
    RT_SCRUNCH_STAGED_VEC = 1,   /* scrunch2_kernel, 16-byte staging loads */
    RT_SCRUNCH_STAGED = 2,       /* scrunch2_kernel, 4-byte staging loads */
    RT_SCRUNCH_GENERAL = 3,      /* scrunch_kernel (explicit-stack pairwise sum) */
    RT_RMED_SMALL = 1,           /* rmed_run_kernel: width <= 255 */
    RT_RMED_LARGE = 2,           /* rmed_large_kernel */
    RT_SUBTRACT_PER_SAMPLE = 1,  /* deredden_subtract_kernel: scrunch factor 1, or 2^31 samples and more */
    RT_SUBTRACT_SLOPE1 = 2,      /* deredden_slope1_kernel: rows off 16 bytes */
    RT_SUBTRACT_SLOPE4 = 3,      /* deredden_slope_kernel: four-sample groups */
    RT_NORM_SCALAR = 1,          /* norm_partial_kernel / norm_apply_kernel */
    RT_NORM_VEC = 2              /* norm_partial4_kernel / norm_apply4_kernel */
};
typedef struct rt_dered_forms {
    uint64_t scrunch_factor;   /* 1: no scrunch */
    uint64_t n_lo;             /* samples the running median runs over */
    uint64_t rmed_width;
    uint32_t scrunch;          /* RT_SCRUNCH_* */
    uint32_t scrunch_chunks;   /* runs of 8192 samples a block's sum is formed from (numpy's buffered reduction) */
    uint32_t rmed;             /* RT_RMED_* */
    uint32_t subtract;         /* RT_SUBTRACT_* */
    uint32_t fused;            /* 1: the subtraction also sums the normalisation's statistics */
    uint32_t norm_partial;     /* RT_NORM_*: the two statistics passes (0 when fused) */
    uint32_t norm_passes;      /* 2: a thread of the statistics grid loads more than once (1 otherwise) */
    uint32_t norm_apply;       /* RT_NORM_* */
} rt_dered_forms;
int rt_deredden_forms(size_t size, size_t width_samples, size_t min_points, int deredden, int normalise,
                      unsigned in_align, unsigned out_align, size_t in_stride, size_t out_stride,
                      rt_dered_forms* forms);

/* ------------------------- peak detection (device) ------------------------ */
/* The data-parallel stages of riptide.peak_detection.find_peaks
 * (peak_detection.py:37-142) over a batch of device periodograms in the
 * rt_periodogram_device layout (trial b at d_snrs + b * snr_stride, L x W
 * row-major).  The host finishes each stage with numpy's own expressions
 * (percentile lerp, polyfit, cluster1d), so the peaks are identical.
 *
 * Order statistics of every (trial, width, segment): segment k covers rows
 * [k * per_seg, (k + 1) * per_seg) (segment_stats, peak_detection.py:71-82);
 * d_out[((b * W + iw) * nseg + k) * nranks + r] = the ranks[r]-th smallest S/N
 * of the segment (NaN if the segment holds a NaN).  per_seg <= 32768. */
int rt_segment_order_stats_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length,
                                  size_t num_widths, size_t nseg, size_t per_seg, const uint32_t* ranks,
                                  size_t nranks, float* d_out, void* stream);
/* Threshold selection (peak_detection.py:131-133): row i of (trial b, width
 * iw) is selected when s > polyval(coeffs[b][iw], logf[i]) and s > smin
 * (fp64, s = float64 of the S/N).  d_coeffs: batch x W x ncoef doubles,
 * highest degree first (np.poly1d order); d_logf: L doubles (np.log of the
 * trial frequencies).  Selected rows are appended, in no particular order, to
 * d_idx[(b * W + iw) * cap ...] and counted in d_counts[b * W + iw] (zeroed
 * by the call); a count above cap means the list was truncated. */
int rt_threshold_select_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length,
                               size_t num_widths, const double* d_logf, const double* d_coeffs, size_t ncoef,
                               double smin, uint32_t* d_counts, uint32_t* d_idx, size_t cap, void* stream);
/* Clustered peaks (find_peaks_single, peak_detection.py:130-141): the
 * selection above, then, along every (trial b, width iw) column,
 *   clusters  the selected rows in ascending order; a new cluster starts at a
 *             selected row i whose previous selected row j has
 *             fabs(d_freqs[i] - d_freqs[j]) > radius (fp64, one rounded
 *             subtraction, strict: cluster1d's np.abs(np.diff(x)) > r);
 *   peak      np.argmax over the cluster in cluster1d's order, ascending
 *             frequency: of the rows attaining the cluster's maximum S/N, the
 *             first (lowest) row on a grid whose frequencies rise with the
 *             row, the last on one where they fall (d_freqs[L - 1] <
 *             d_freqs[0], a periodogram's own grid).  The grid must be
 *             monotone.
 * d_freqs: L doubles, the trial frequencies 1 / periods; radius: clrad / tobs.
 * A NaN S/N is never selected, +inf is selected like any value.
 * The k-th cluster's peak, clusters in ascending row order, is left in
 * d_rows[(b * W + iw) * cap + k] and d_snr[(b * W + iw) * cap + k], the
 * number of clusters in d_counts[b * W + iw]; a count above cap means the
 * first cap records are valid and the column was truncated (nothing is
 * written past them).  chunk_rows: rows one workgroup walks (0 = default,
 * rounded up to a multiple of 64, at most 2^20); the result does not depend
 * on it.  d_workspace: rt_find_peaks_workspace_bytes bytes, 8-byte aligned.
 * Stream-ordered, no host synchronisation.  RT_EINVAL (nothing is launched)
 * for: cap == 0, ncoef == 0 or > 64, length >= 2^32, batch > 65535,
 * batch * num_widths >= 2^31, a workspace below
 * rt_find_peaks_workspace_bytes.  batch, length or num_widths of 0 is RT_OK
 * (length 0: the counts are zeroed). */
int rt_find_peaks_workspace_bytes(size_t batch, size_t length, size_t num_widths, size_t chunk_rows, size_t* bytes);
int rt_find_peaks_device(const float* d_snrs, size_t batch, size_t snr_stride, size_t length, size_t num_widths,
                         const double* d_logf, const double* d_freqs, const double* d_coeffs, size_t ncoef,
                         double smin, double radius, uint32_t* d_counts, uint32_t* d_rows, float* d_snr,
                         size_t cap, size_t chunk_rows, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host only, no device: the same walk over one trial's host arrays (snrs: L x
 * W row-major; coeffs: W x ncoef; counts: W; rows, snr: W x cap) -- the
 * specification the kernels are pinned to. */
int rt_find_peaks_host(const float* snrs, size_t length, size_t num_widths, const double* logf, const double* freqs,
                       const double* coeffs, size_t ncoef, double smin, double radius,
                       uint32_t* counts, uint32_t* rows, float* snr, size_t cap);

/* ------------------------- candidate folding ------------------------------ */
/* riptide/folding.py:19-81 (what TimeSeries.fold returns) for a batch of
 * candidates, bit-identical to the reference's arithmetic: the series
 * downsampled by `factor`, cut into m = floor(size / factor) / bins whole
 * periods, scaled by (float)pow(m * factor, -0.5), then
 *   subints == 1 or m == 1        the float32 sum over the m rows: bins floats
 *   subints == 0 (None) or == m   the (m, bins) rows themselves
 *   any other subints             the rows downsampled along their first axis
 *                                 by m / subints: floor(m / (m / subints)) rows,
 *                                 which is subints - 1 for some (m, subints)
 *                                 pairs, as in the reference.
 * Candidates of one call may fold different series (rows of d_data). */
typedef struct rt_fold_spec {
    double   factor;    /* period / bins / tsamp, must be > 1 and <= size */
    uint64_t out_off;   /* float offset of this candidate's result in d_out */
    uint32_t series;    /* row of d_data */
    uint32_t bins;      /* >= 2 */
    uint32_t subints;   /* 0 = None */
    uint32_t reserved;
} rt_fold_spec;

/* Host only, no device: the whole periods m and the rows of the result
 * (*rows == 0: a 1-D profile of `bins` floats).  RT_EINVAL as below. */
int rt_fold_shape(size_t size, double factor, size_t bins, size_t subints, size_t* m, size_t* rows);
/* Host only: device workspace bytes of a call with these specs (the
 * descriptor tables and the row arrays of the candidates whose result is not
 * the row array itself).  Validates factor, bins, m and subints. */
int rt_fold_workspace_bytes(size_t size, const rt_fold_spec* specs, size_t nspecs, size_t* bytes);
/* Fold `nspecs` candidates of the `nseries` device-resident series (series r
 * at d_data + r * data_stride) into d_out.  Stream-ordered, no host
 * synchronisation.  `specs` is host memory and is read before the call
 * returns: the descriptor tables are built in a pinned staging buffer that the
 * library owns and reuses only after the stream has passed the copy, so the
 * caller may free or overwrite `specs` at once.  The staging buffers and
 * their events live for the rest of the process (a few KiB each, as many as
 * calls were ever in flight at once); they are not released when the library
 * is unloaded.  d_data, d_out and
 * d_workspace must stay valid until the stream has run the call.
 * RT_EINVAL (nothing is launched) for: a factor outside (1, size], bins < 2,
 * m == 0, subints > m, series >= nseries, a result range past out_floats or
 * overlapping another spec's, a workspace below rt_fold_workspace_bytes.
 * nspecs == 0 is RT_OK. */
int rt_fold_device(const float* d_data, size_t size, size_t data_stride, size_t nseries,
                   const rt_fold_spec* specs, size_t nspecs, float* d_out, size_t out_floats,
                   void* d_workspace, size_t workspace_bytes, void* stream);
/* Host-buffer form: uploads the `nseries` contiguous series of x once, folds
 * every candidate, copies out_floats floats back.  Synchronous. */
int rt_fold(const float* x, size_t size, size_t nseries, const rt_fold_spec* specs, size_t nspecs,
            float* out, size_t out_floats);

/* ------------------------- candidate refinement ---------------------------- */
/* The search over small period and DM offsets that follows a sub-band fold:
 * the sub-bands and the sub-integrations of a folded cube are re-aligned by
 * whole bins and the boxcar S/N of every trial's profile is taken.  For a cube
 * x[b][s][n] (float32, B bands, S sub-integrations, N bins), shift tables
 * dshift[k][b] (K DM trials) and pshift[j][s] (J period trials) with entries in
 * [0, N), W widths in [1, N - 1] and stdnoise > 0:
 *   y[k][s][n]    = sum over b = 0..B-1 of x[b][s][(n + dshift[k][b]) mod N]
 *   prof[k][j][n] = sum over s = 0..S-1 of y[k][s][(n + pshift[j][s]) mod N]
 *   snr[k][j][w]  = snr1 of prof[k][j][:] at width w with stdnoise
 * The sums are float32, start from 0.0f and add in index order: host and
 * device profiles have the same bits.  The S/N's prefix sums are taken in
 * another order on the device: S/N agrees to rounding, not to bits. */

/* Host only, the physics in double (operation order: refine_host.hpp):
 *   pshift[j][s] = floor(N*T*(1/P - 1/P_j) * ((s + 0.5)/S - 0.5) + 0.5)          mod N
 *   dshift[k][b] = floor(N * kdm*(DM_k - DM)*(f[b]^-2 - fmax^-2) / P + 0.5)      mod N
 * P: the fold period; T: the fold's span in seconds (m * P, m of rt_fold_shape);
 * f: band centre frequencies in MHz, fmax their maximum; DM: the fold's.
 * pshift: J x S, dshift: K x B, int32 in [0, N).  RT_EINVAL for P, T, a trial
 * period or a frequency that is not positive and finite, N < 2, S, B, J or K
 * of 0, a shift of magnitude 2^31 or more before the reduction (a trial DM
 * that is not finite is one). */
int rt_refine_shifts(double period, double span, size_t bins, size_t subints, const double* band_freqs,
                     size_t bands, double dm, double kdm, const double* periods, size_t nper, const double* dms,
                     size_t ndm, int32_t* pshift, int32_t* dshift);

/* Host only: the specification above for one candidate, sequential, with
 * snr1's prefix sums (a double accumulator stored as float32).  snr: K x J x W;
 * prof: K x J x N, or NULL.  RT_EINVAL for N < 2, a count of 0, a shift
 * outside [0, N), a width outside [1, N - 1] and stdnoise <= 0 (the last two
 * with snr1's texts). */
int rt_refine_host(const float* cube, size_t bands, size_t subints, size_t bins, const int32_t* dshift, size_t ndm,
                   const int32_t* pshift, size_t nper, const uint32_t* widths, size_t num_widths, float stdnoise,
                   float* snr, float* prof);

/* One candidate of a batched call: where its arrays lie in the call's packed
 * buffers, and its shape.  Candidates of different shapes share a call. */
typedef struct rt_refine_spec {
    uint64_t cube_off;    /* float offset of the cube [bands][subints][bins] in cubes */
    uint64_t dshift_off;  /* int32 offset of dshift [ndm][bands] in shifts */
    uint64_t pshift_off;  /* int32 offset of pshift [nper][subints] in shifts */
    uint64_t width_off;   /* uint32 offset of the nw widths in widths */
    uint64_t snr_off;     /* float offset of the result [ndm][nper][nw] in snr */
    uint64_t prof_off;    /* float offset of [ndm][nper][bins] in profiles (unused without profiles) */
    uint32_t bands, subints;
    uint32_t bins;        /* 2 .. 1024 */
    uint32_t ndm, nper, nw;
    float    stdnoise;
    uint32_t reserved;
} rt_refine_spec;

/* Host only: device workspace bytes of a call with these specs (the
 * descriptor table and y of every candidate).  Validates the shapes. */
int rt_refine_workspace_bytes(const rt_refine_spec* specs, size_t nspecs, size_t* bytes);
/* Refine `nspecs` candidates whose arrays are device resident.  Stream-ordered:
 * no host synchronisation and no device allocation; `specs` is host memory,
 * read before the call returns through a pinned staging buffer the library
 * owns (as rt_fold_device).  d_profiles may be NULL.  The buffers carry no
 * lengths: the caller answers for every offset of `specs` lying inside them.
 * Device tables are not validated and cannot cause a read outside the cube:
 * a shift v is used as (uint32_t)v mod bins, a width is clamped to
 * [1, bins - 1].  RT_EINVAL (nothing is launched) for bins outside [2, 1024],
 * a count of 0, stdnoise <= 0, a null pointer, a workspace below
 * rt_refine_workspace_bytes.  nspecs == 0 is RT_OK. */
int rt_refine_device(const float* d_cubes, const int32_t* d_shifts, const uint32_t* d_widths,
                     const rt_refine_spec* specs, size_t nspecs, float* d_snr, float* d_profiles,
                     void* d_workspace, size_t workspace_bytes, void* stream);
/* Host-buffer form: validates every table as rt_refine_host does, uploads the
 * arrays once (their lengths: the furthest end any spec names), runs every
 * candidate, copies the S/N (and the profiles, unless NULL) back.  Synchronous. */
int rt_refine(const float* cubes, const int32_t* shifts, const uint32_t* widths, const rt_refine_spec* specs,
              size_t nspecs, float* snr, float* profiles);

/* --------------------------- single-pulse search --------------------------- */
/* Boxcar matched filtering of B series x[b][0..N) (float32, rows ldx floats
 * apart, assumed dereddened and normalised to unit variance) at K widths
 * w[0..K) in samples, strictly ascending:
 *   s[b][k][t] = float32( sum of x[b][t .. t + w_k) / sqrt((double)w_k) )   0 <= t <= N - w_k
 * The sum is formed in float64 from partial sums in a pinned order
 * (pulse_host.hpp: sequential runs of 16 samples, the run totals added in
 * order, the partial sums restarting every RT_PULSE_SEGMENT samples; a window
 * that crosses restarts is its head, the whole segments between and its tail,
 * added in that order).  Host and device results have the same bits.
 *   c_k = w_k / 2 (integer);  best[b][t] = max over k of s[b][k][t - c_k] over
 *   the widths whose window [t - c_k, t - c_k + w_k) lies inside the row,
 *   kbest[b][t] the smallest k attaining it (float compares: a NaN never
 *   wins); no width fits: best = -inf, kbest = -1.
 * (b, t) is an event iff best[b][t] >= threshold, best[b][t] > best[b][u] for
 * every u in [t - R, t) and best[b][t] >= best[b][u] for every u in (t, t + R]
 * (u clipped to the row).  Events are listed in (b, t) order.
 * RT_EINVAL for K == 0, a width < 1, widths not strictly ascending, the
 * largest width > N, a width or radius above RT_PULSE_MAX_WIDTH, a threshold
 * that is not finite, ldx < N, N above RT_PULSE_MAX_SAMPLES. */
#define RT_PULSE_MAX_WIDTH 6144
#define RT_PULSE_SEGMENT 1024
#define RT_PULSE_MAX_SAMPLES 1073741824
typedef struct rt_pulse_event {
    int32_t series;   /* b */
    int32_t sample;   /* t */
    int32_t iwidth;   /* kbest[b][t] */
    float   snr;      /* best[b][t] */
} rt_pulse_event;

/* Host only: the specification, sequential.  events: room for `capacity`
 * records (NULL when capacity == 0); the first `capacity` events are written,
 * *count (if not NULL) is the number found, never cut.  best (float32 [B][N])
 * and kbest (int32 [B][N]) are written unless NULL. */
int rt_single_pulse_host(const float* x, size_t nseries, size_t size, size_t ldx, const int32_t* widths,
                         size_t num_widths, float threshold, size_t radius, rt_pulse_event* events, size_t capacity,
                         uint64_t* count, float* best, int32_t* kbest);
/* Host only: the device form's tile length in samples (*tile; a launch works on
 * tiles of this many outputs with a halo of radius + largest width on each
 * side) and RT_PULSE_MAX_WIDTH (*max_width). */
int rt_single_pulse_limits(size_t* tile, size_t* max_width);
/* Host only, read-only: the device form's LDS plan for a largest width `wmax`
 * and a radius (pulse_plan, pulse_host.hpp; neither the series nor their
 * number enter it).  *chunk: the outputs, halo included, whose partial sums
 * are in LDS at once, a multiple of RT_PULSE_SEGMENT; *chunk_segs: the
 * segments those need; *lds_bytes: the workgroup's dynamic LDS.  Any pointer
 * may be NULL.  RT_EINVAL for wmax < 1, wmax or radius above
 * RT_PULSE_MAX_WIDTH. */
int rt_single_pulse_plan(size_t wmax, size_t radius, size_t* chunk, size_t* chunk_segs, size_t* lds_bytes);
/* Host only: device workspace bytes of a call of this shape. */
int rt_single_pulse_workspace_bytes(size_t nseries, size_t size, size_t num_widths, size_t capacity, size_t* bytes);
/* The same search of device-resident series.  Stream-ordered: no host
 * synchronisation and no device allocation; `widths` is host memory, read
 * before the call returns through a pinned staging buffer the library owns.
 * d_events: room for `capacity` records (may be NULL when capacity == 0);
 * *d_count (uint64, device) becomes the number of events found.  When that is
 * above capacity the records written are not specified: call again with room
 * for *d_count.  Otherwise d_events[0 .. *d_count) is the host function's
 * list, in the same order on every run.  d_best / d_kbest: [B][N] contiguous,
 * or NULL.  Also RT_EINVAL (nothing is launched) for nseries > 65535, a null
 * pointer, a workspace below rt_single_pulse_workspace_bytes.  nseries == 0
 * is RT_OK with *d_count = 0. */
int rt_single_pulse_device(const float* d_x, size_t nseries, size_t size, size_t ldx, const int32_t* widths,
                           size_t num_widths, float threshold, size_t radius, rt_pulse_event* d_events,
                           size_t capacity, uint64_t* d_count, float* d_best, int32_t* d_kbest, void* d_workspace,
                           size_t workspace_bytes, void* stream);

/* ------------------- resampling (the acceleration search) ------------------ */
/* Time-domain resampling of series x[B][0..N) (float32, rows ldx floats
 * apart): output row r (rows ldo floats apart) is source row src[r] stretched
 * by the float64 factor f = factor[r], nearest neighbour:
 *   q_j = j * (N - j)                          exact, j = 0 .. N - 1
 *   s_j = (int64) rint(f * (double)q_j)        one IEEE double multiply, round-half-even
 *   out[r][j] = x[src[r]][clamp(j - s_j, 0, N - 1)]
 * a copy of the float's bits (NaN payloads, -0.0 and denormals included), so
 * host and device results have the same bits.  With f = accel * tsamp / (2 c),
 * accel in m/s^2 positive when the source accelerates away, a uniformly
 * accelerated signal becomes strictly periodic at its mid-observation
 * frequency.  f = 0 is a copy.  out must not overlap x.
 * RT_EINVAL (nothing is written or launched) for N above
 * RT_RESAMPLE_MAX_SAMPLES (q_j must stay exact in a double), R above
 * RT_RESAMPLE_MAX_ROWS, and, when R * N > 0: a null pointer, ldx < N, ldo < N,
 * a src[r] outside [0, B), a factor that is not finite or has
 * fabs(f) * (double)N >= 1.0 (below that the map is monotone).  R == 0 or
 * N == 0 is RT_OK and does nothing. */
#define RT_RESAMPLE_MAX_SAMPLES 134217728
#define RT_RESAMPLE_MAX_ROWS 65535
/* Host only: the specification, sequential. */
int rt_resample_host(const float* x, size_t nseries, size_t size, size_t ldx, const int32_t* src,
                     const double* factor, size_t nrows, float* out, size_t ldo);
/* The same map of device-resident series.  Stream-ordered: no host
 * synchronisation, no device allocation and no workspace; src and factor are
 * host memory, read before the call returns (they travel as kernel
 * arguments, RT_RESAMPLE_LAUNCH_ROWS rows a launch). */
#define RT_RESAMPLE_LAUNCH_ROWS 128
int rt_resample_device(const float* d_x, size_t nseries, size_t size, size_t ldx, const int32_t* src,
                       const double* factor, size_t nrows, float* d_out, size_t ldo, void* stream);

/* --------------------------- harmonic flagging ----------------------------- */
/* riptide/pipeline/harmonic_testing.py (hdiag, htest) and the pair loop of
 * Pipeline.flag_harmonics (pipeline/pipeline.py:217-249).  A cluster is its
 * centre's (freq, snr, ducy, dm) in fp64; F is the postulated fundamental, H
 * the postulated harmonic.  Every value is computed with the reference's own
 * sequence of fp64 operations; the closest fraction is exactly
 * Fraction(fast.freq / slow.freq).limit_denominator(denom_max).
 * Supported range (RT_EINVAL outside it, nothing is launched): finite
 * positive freq and ducy, tobs > 0, 1 <= denom_max <= 1024, and every
 * frequency ratio below 2^40. */
typedef struct rt_htest_params {
    double   tobs;                 /* integration time, s */
    double   band;                 /* abs(fmin ** -2 - fmax ** -2), computed by the caller */
    double   phase_distance_max;
    double   dm_distance_max;
    double   snr_distance_max;
    uint32_t denom_max;
} rt_htest_params;

/* Host only, no device: hdiag for the npairs pairs (F = cluster pi[k], H =
 * cluster pj[k]) of n clusters: the fraction H.freq / F.freq as num / den and
 * the three distances.  Bit-identical to the reference on the same machine
 * (the square root of num * den is libm's pow(x, 0.5), CPython's int ** 0.5). */
int rt_hdiag_host(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                  const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params,
                  int64_t* num, int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance);
/* The same outputs computed by the device (host buffers, synchronous).  num,
 * den, phase_distance and dm_distance equal rt_hdiag_host's bit for bit;
 * snr_distance uses the device's sqrt and is within
 * 8 * 2^-52 * max(|F.snr|, |H.snr|) of it. */
int rt_hdiag_pairs(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                   const int32_t* pi, const int32_t* pj, size_t npairs, const rt_htest_params* params,
                   int64_t* num, int64_t* den, double* phase_distance, double* dm_distance, double* snr_distance);
/* Flag the harmonics among n clusters given in rank order (decreasing S/N):
 * the reference's loop over itertools.combinations, which skips a pair when
 * either member is already a harmonic.  parent[j] = rank of j's fundamental
 * or -1; hnum[j] / hden[j] = H.freq / F.freq for a flagged j, 0 / 0 otherwise.
 * The device tests every pair (i, j > i) tile by tile of block_rows rows
 * (0 = default) into a bit matrix; the host re-decides with rt_hdiag_host's
 * arithmetic each pair whose S/N distance is within the guard band of its
 * bound, then resolves the rows in rank order.  The result equals the host
 * loop's and does not depend on block_rows.  Device and pinned workspace: two
 * tiles of at most 4 MiB of words + 32 KiB of pair list each, plus 32 n bytes
 * of inputs on the device.  n <= 2^24; n <= 1 is RT_OK and tests nothing. */
int rt_flag_harmonics(const double* freq, const double* snr, const double* ducy, const double* dm, size_t n,
                      const rt_htest_params* params, size_t block_rows, int32_t* parent, int64_t* hnum,
                      int64_t* hden);
/* Counters of this thread's last rt_flag_harmonics: tiles run, pairs the host
 * re-decided from the near lists, rows decided wholly on the host because
 * their tile's near list overflowed, and the pair kernel's summed time in
 * milliseconds (HIP events).  Any pointer may be NULL. */
int rt_flag_harmonics_stats(uint64_t* tiles, uint64_t* near_pairs, uint64_t* host_rows, double* kernel_ms);

/* ------------------------ incoherent dedispersion -------------------------- */
/* Channelised data (SIGPROC filterbank order: time-major [nsamp, nchans], the
 * channel fastest) summed along the dispersion sweep of each trial DM:
 *   out[d, t] = sum over unmasked channels c of x[t + delay[d, c], c]
 * Sample type codes: */
#define RT_DEDISP_U8  0
#define RT_DEDISP_I8  1
#define RT_DEDISP_F32 2
/* 8-bit sums are exact integers in float32 while 255 * nchans < 2^24 */
#define RT_DEDISP_MAX_CHANS_8BIT 65793
/* Packed sample types, a range of their own (the code is 0x100 + nbits).  x /
 * d_block is then bytes, [nsamp, row_bytes] with row_bytes = nchans * nbits /
 * 8 (nchans * nbits must be a multiple of 8: RT_EINVAL "rows are not a whole
 * number of bytes" otherwise), and only byte-aligned.  One definition for
 * host and device:
 *   1, 2, 4 bit  unsigned, SIGPROC's packing, least significant bits first:
 *                channel c of a row is
 *                (row[(c * nbits) >> 3] >> ((c * nbits) & 7)) & (2^nbits - 1)
 *   16 bit       unsigned, little-endian: row[2c] | row[2c + 1] << 8
 * (a most-significant-bit-first packing is not supported).  Every
 * rt_dedisperse*, rt_zero_dm_mean_* and rt_channel_stats_* entry point takes
 * these codes.  1/2/4-bit data is summed as 8-bit data is: exact integers,
 * at most RT_DEDISP_MAX_CHANS_8BIT channels.  16-bit data is converted
 * exactly and summed in float32 in channel order, as float data is (so exact
 * up to 256 channels; no channel cap).  With RT_DEDISP_ZERO_DM, S[t] is an
 * exact integer for all four widths, so m and y are reproducible bit for bit.
 * The statistics are integers, exact below 2^53. */
#define RT_DEDISP_U1  0x101
#define RT_DEDISP_U2  0x102
#define RT_DEDISP_U4  0x104
#define RT_DEDISP_U16 0x110
/* Host only: *bytes = the bytes of one time sample's row of nchans channels,
 * for the three plain codes (nchans, nchans, 4 * nchans) and the packed ones
 * (nchans * nbits / 8).  RT_EINVAL for an unknown code, nchans == 0, a NULL
 * bytes, or packed rows that are not a whole number of bytes. */
int rt_dedisp_row_bytes(int dtype, size_t nchans, size_t* bytes);

/* Host only, no device: the delay table, in samples, against the highest
 * frequency f_ref = max(freqs_mhz).  In float64, in this order:
 *   a = 1.0 / (f * f) - 1.0 / (f_ref * f_ref)
 *   delay[d, c] = (int64) floor(kdm * dm[d] * a / tsamp + 0.5)
 * kdm is the dispersion constant in s MHz^2 cm^3 / pc (1 / 2.41e-4 in the
 * PRESTO / pulsar-timing convention).  *max_delay (may be NULL) is the largest
 * entry.  RT_EINVAL for nchans == 0 or ndm == 0, a frequency that is not
 * positive and finite, a DM that is negative or not finite, tsamp <= 0, or a
 * delay of 2^31 samples or more. */
int rt_dedisperse_delays(const double* freqs_mhz, size_t nchans, const double* dms, size_t ndm, double tsamp,
                         double kdm, int64_t* delays, int64_t* max_delay);
/* Host only, no device: the specification the kernels are pinned to.  x is
 * [nsamp, nchans] of the sample type, delays [ndm, nchans] with every entry in
 * [0, max_delay], mask NULL or [nchans] with non-zero = channel skipped, out
 * [ndm, nout].  8-bit data is summed in int32, float data in float32 in
 * channel order.  RT_EINVAL when nout + max_delay > nsamp, a delay lies outside
 * [0, max_delay], the type code is unknown, or 8-bit data has more than
 * RT_DEDISP_MAX_CHANS_8BIT channels. */
int rt_dedisperse_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                       const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out);
/* Device workspace bytes of rt_dedisperse_device for a block of nsamp_blk
 * samples: the block transposed to channel-major, rows padded to 16 bytes
 * (1/2/4-bit data: the size of 8-bit data of the same shape, the rows are
 * unpacked; 16-bit data: the size of float32 data). */
int rt_dedisperse_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, size_t* bytes);
/* One resident block of nsamp_blk time samples, d_block [nsamp_blk, nchans]:
 * writes d_out[d * out_stride + out_offset + t] for t in [0, nsamp_blk -
 * max_delay), exactly the outputs whose reads all fall inside the block.
 * d_delays is int32 [ndm, nchans] (entries are clamped to [0, max_delay]),
 * d_mask NULL or uint8 [nchans].  Stream-ordered, no host synchronisation; no
 * load leaves the block or the workspace.  d_block must be aligned to its
 * sample type, d_workspace to 16 bytes.  8-bit results are exact; float32
 * results are summed in channel order.  RT_EINVAL (nothing is launched) for
 * an unknown type code, nchans == 0, ndm == 0, max_delay outside [0,
 * nsamp_blk), nsamp_blk >= 2^31, out_stride < out_offset + nsamp_blk -
 * max_delay, 8-bit data with more than RT_DEDISP_MAX_CHANS_8BIT channels, a
 * NULL or misaligned pointer, or a workspace below
 * rt_dedisperse_workspace_bytes. */
int rt_dedisperse_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const int32_t* d_delays,
                         const uint8_t* d_mask, size_t ndm, int64_t max_delay, float* d_out, size_t out_stride,
                         size_t out_offset, void* d_workspace, size_t workspace_bytes, void* stream);
/* Host only, read-only, no device call: which of its two read paths the sum
 * kernel of rt_dedisperse_device takes for one channel of one tile of 16 DMs x
 * 256 outputs (dedisp_span, dedisp_types.hpp: the kernel's own rule).  esize
 * is the bytes of a workspace row's element: 1 for 8-bit and 1/2/4-bit data, 4
 * for float32 and 16-bit data and for every type under RT_DEDISP_ZERO_DM.  lo
 * and hi are the smallest and largest delay, clamped to [0, max_delay], of the
 * tile's 16 DM rows in that channel (a partial tile repeats the last DM).
 * *ndw: the dwords from the one holding the first element read to the last
 * one read, (256 + hi - (lo & ~3) + 3) / 4 for esize 1 and 256 + hi - lo for
 * esize 4.  *staged: 1 when they are staged in LDS, ndw <= 264 (esize 1: hi -
 * (lo & ~3) <= 800) or ndw <= 520 (esize 4: hi - lo <= 264); 0 when the
 * channel is read from the workspace row directly.  Both paths give the same
 * bits.  Either pointer may be NULL.  RT_EINVAL for an esize other than 1 or
 * 4, lo < 0, lo > hi, hi >= 2^31. */
int rt_dedisperse_span_plan(size_t esize, int64_t lo, int64_t hi, size_t* ndw, int* staged);
/* Host-buffer form: uploads x [nsamp, nchans], the delays (int64, as
 * rt_dedisperse_delays writes them) and the mask, runs the kernels, copies out
 * [ndm, nsamp - max_delay] back.  Synchronous. */
int rt_dedisperse(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays, const uint8_t* mask,
                  size_t ndm, int64_t max_delay, float* out);

/* ---- RFI mitigation in front of the sum: zero-DM filter, channel statistics */
/* Flag of the _opt forms below: the zero-DM filter (Eatough, Keane & Lyne
 * 2009), every time sample minus its mean over the unmasked channels U, Nu =
 * |U|, before the sum.  One definition for host and device:
 *   S[t]      = sum over c in U of x[t, c]     8-bit: an exact integer;
 *               float32: accumulated in float64 (the host in ascending channel
 *               order, the device in its own fixed order)
 *   m[t]      = (float32)(S[t] / Nu)           divided in float64, rounded once
 *   y[t, c]   = (float32)x[t, c] - m[t]        one float32 subtraction; int8
 *                                              samples enter as signed values
 *   out[d, t] = sum over c in U of y[t + delay[d, c], c]
 *               float32 additions in channel order
 * Nu == 0 gives m = 0 and out = 0.  For 8-bit data m and y are reproducible
 * bit for bit; only the last sum carries a rounding bound. */
#define RT_DEDISP_ZERO_DM 1u
/* The four entry points above with a flags argument (0 or RT_DEDISP_ZERO_DM;
 * any other bit is RT_EINVAL).  flags == 0 is the plain call, bit for bit.
 * With RT_DEDISP_ZERO_DM every sample type takes the float32 path: the
 * workspace is nchans float32 rows of the padded pitch plus nsamp_blk floats
 * for m (16-byte aligned), and 8-bit data is still refused above
 * RT_DEDISP_MAX_CHANS_8BIT channels. */
int rt_dedisperse_host_opt(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                           const uint8_t* mask, size_t ndm, int64_t max_delay, size_t nout, float* out,
                           uint32_t flags);
int rt_dedisperse_workspace_bytes_opt(int dtype, size_t nsamp_blk, size_t nchans, uint32_t flags, size_t* bytes);
int rt_dedisperse_device_opt(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                             const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, int64_t max_delay,
                             float* d_out, size_t out_stride, size_t out_offset, void* d_workspace,
                             size_t workspace_bytes, void* stream, uint32_t flags);
int rt_dedisperse_opt(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                      const uint8_t* mask, size_t ndm, int64_t max_delay, float* out, uint32_t flags);
/* ---- sub-band sums: every band of a table from one pass over the block */
/* A band is a half-open channel range [lo, hi); bands is uint32 [nbands][2].
 * Bands may overlap, be empty, come in any order and cover the whole file:
 *   out[d, b, t] = sum over unmasked c in [lo_b, hi_b) of x[t + delay[d, c], c]
 * The delays are those of the plain call, against the highest frequency of the
 * whole file, so the bands stay aligned with each other.  The sums are the
 * plain call's: exact integers for 8-bit and 1/2/4-bit data, float32 additions
 * in ascending channel order within the band for float and 16-bit data; the
 * row of the band [0, nchans) is the plain call's row, bit for bit.  With
 * RT_DEDISP_ZERO_DM m[t] is still the mean over the unmasked channels of the
 * whole file, and y is summed in float32 over the band.  A band with no
 * unmasked channel gives zeros.
 * The device call takes at most RT_DEDISP_MAX_BANDS bands (a grid layer each). */
#define RT_DEDISP_MAX_BANDS 65535
/* Host only, no device: the specification.  rt_dedisperse_host_opt with a band
 * table, out [ndm, nbands, nout].  RT_EINVAL for a band with lo > hi or hi >
 * nchans, a NULL bands with nbands > 0, and everything rt_dedisperse_host_opt
 * refuses; nbands == 0 writes nothing. */
int rt_dedisperse_bands_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                             const uint8_t* mask, size_t ndm, const uint32_t* bands, size_t nbands,
                             int64_t max_delay, size_t nout, float* out, uint32_t flags);
/* rt_dedisperse_device_opt with a band table in device memory, d_bands uint32
 * [nbands][2] (4-byte aligned): writes d_out[(d * nbands + b) * out_stride +
 * out_offset + t] for t in [0, nsamp_blk - max_delay).  The band edges are
 * clamped as they are read, hi to nchans and lo to hi, as delays are clamped:
 * no load leaves the block or the workspace.  The workspace is that of
 * rt_dedisperse_workspace_bytes_opt.  RT_EINVAL (nothing is launched) for
 * nbands == 0, nbands > RT_DEDISP_MAX_BANDS, ndm * nbands >= 2^32, a NULL
 * d_bands, and everything rt_dedisperse_device_opt refuses. */
int rt_dedisperse_bands_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, const uint32_t* d_bands,
                               size_t nbands, int64_t max_delay, float* d_out, size_t out_stride, size_t out_offset,
                               void* d_workspace, size_t workspace_bytes, void* stream, uint32_t flags);
/* Host-buffer form, as rt_dedisperse_opt: out [ndm, nbands, nsamp - max_delay].
 * Synchronous.  Also RT_EINVAL for a band with lo > hi or hi > nchans. */
int rt_dedisperse_bands(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                        const uint8_t* mask, size_t ndm, const uint32_t* bands, size_t nbands, int64_t max_delay,
                        float* out, uint32_t flags);
/* Host only, no device: the zero-DM mean series m [nsamp] of x [nsamp, nchans]
 * as defined above (mask NULL or [nchans], non-zero = channel skipped).
 * RT_EINVAL for an unknown type code, nchans == 0, or 8-bit data of more than
 * RT_DEDISP_MAX_CHANS_8BIT channels. */
int rt_zero_dm_mean_host(const void* x, int dtype, size_t nsamp, size_t nchans, const uint8_t* mask, float* m);
/* The same series of one resident block, d_m float32 [nsamp_blk]: the
 * row-mean kernel alone.  Stream-ordered; no load leaves the block. */
int rt_zero_dm_mean_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, const uint8_t* d_mask,
                           float* d_m, void* stream);
/* Host only, no device: ADDS the per-channel sums of x [nsamp, nchans] into
 * acc, float64 [2, nchans]: acc[0][c] += sum over t of x[t, c], acc[1][c] +=
 * sum over t of x[t, c]^2 (int8 samples as signed values), in time order.
 * A file is streamed block by block into zeroed accumulators; 8-bit sums are
 * integers, exact below 2^53. */
int rt_channel_stats_host(const void* x, int dtype, size_t nsamp, size_t nchans, double* acc);
/* Device workspace bytes of rt_channel_stats_device: the per-chunk partial
 * sums. */
int rt_channel_stats_workspace_bytes(size_t nsamp_blk, size_t nchans, size_t* bytes);
/* The same addition for one resident block into d_acc, float64 [2, nchans] in
 * device memory: per-chunk partial sums to the workspace, folded into d_acc
 * in chunk order by a second kernel.  No floating-point atomics: the same
 * input gives the same bits.  Stream-ordered.  d_acc and d_workspace must be
 * 8-byte aligned. */
int rt_channel_stats_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, double* d_acc,
                            void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- the block mask: interference narrow in frequency and intermittent in time */
/* A mask in time and frequency.  Time is cut into blocks of block_len samples,
 * block b the absolute samples [b * block_len, (b + 1) * block_len) of the
 * observation; cells is uint8 [nblocks, nchans], non-zero = that channel is
 * flagged during that block.  fill holds one value per channel in the sample's
 * own type: uint8 [nchans] for RT_DEDISP_U8, int8 for RT_DEDISP_I8, float32
 * for RT_DEDISP_F32 (4-byte aligned), uint16 for RT_DEDISP_U16 (2-byte
 * aligned), and for the 1/2/4-bit types uint8 [nchans], one unpacked value per
 * byte of which only the low nbits bits are used.  Every bit pattern is a
 * valid sample: nothing is range-checked.  t_origin is the absolute sample
 * index of row 0 of the block or gulp the call is given.  The mask is a pure
 * replacement in front of everything else:
 *   x'[t, c] = fill[c]  if cells[(t_origin + t) / block_len, c] != 0
 *              x[t, c]  otherwise
 * and every other definition of this header (the channel mask, the zero-DM
 * mean over the unmasked channels, y = x' - m, the sums, the band sums, the
 * exactness of integer data) is applied to x' unchanged; a channel the channel
 * mask skips stays skipped whatever its cells say.  So rt_block_replace_host
 * followed by the existing host specification is the specification of the
 * _cells calls below, and the device gives the bits of its plain call on x'.
 * A NULL pointer to the struct means no block mask.  A call whose rows reach
 * past the mask, t_origin + nsamp > nblocks * block_len, is RT_EINVAL, as are
 * block_len == 0, a NULL cells or fill, and t_origin + nsamp >= 2^64 (the
 * sum is formed in 64 bits): no load leaves the cells.  The
 * kernels index the cells in 64 bits: nblocks * nchans has no limit of its
 * own.  The mask needs no workspace (rt_dedisperse_workspace_bytes_opt is
 * unchanged).  The host-buffer calls rt_dedisperse, rt_dedisperse_opt and
 * rt_dedisperse_bands take no block mask. */
typedef struct rt_block_mask {
    const uint8_t* cells;      /* [nblocks, nchans] */
    size_t         nblocks;
    size_t         block_len;  /* >= 1 */
    uint64_t       t_origin;
    const void*    fill;       /* [nchans], the sample's own type */
} rt_block_mask;
/* Host only, no device: the specification of the replacement.  out = x' in
 * x's own format (packed rows stay packed), [nsamp, row_bytes of
 * rt_dedisp_row_bytes]; out may be x.  cells and fill are host arrays.  A NULL
 * bm copies.  RT_EINVAL for an unknown type code, nchans == 0, packed rows
 * that are not whole bytes, and a mask refused as above. */
int rt_block_replace_host(const void* x, int dtype, size_t nsamp, size_t nchans, const rt_block_mask* bm, void* out);
/* Host only, no device: WRITES stats, float64 [nblk, 2, nchans] with nblk =
 * ceil(nsamp / block_len): stats[b][0][c] the sum and stats[b][1][c] the sum
 * of squares of x[t, c] over the rows of block b, blocks counted from row 0
 * of x (the last one may be partial; int8 samples as signed values).  Integer
 * samples give exact integers.  In float64 the order is fixed, and the device
 * follows it, so both give the same bits for every sample type: a block is cut
 * into chunks of 2048 rows from its first row; within a chunk row j (from 0)
 * is added to partial sum j mod 4, each from 0.0 in row order; the chunk's sum
 * is ((p0 + p1) + p2) + p3; the block's sum is the chunks' sums added in
 * order from 0.0.  A square is one float64 product (exact for float32 and
 * 16-bit samples).  RT_EINVAL for block_len == 0, an unknown type code and
 * nchans == 0. */
int rt_block_stats_host(const void* x, int dtype, size_t nsamp, size_t nchans, size_t block_len, double* stats);
/* Device workspace bytes of rt_block_stats_device: none for block_len <= 2048,
 * the per-chunk partial sums of longer blocks otherwise. */
int rt_block_stats_workspace_bytes(size_t nsamp_blk, size_t nchans, size_t block_len, size_t* bytes);
/* The same statistics of one resident block into d_stats, float64 [nblk, 2,
 * nchans] in device memory (written, not accumulated), bit for bit the host's.
 * No atomics.  Stream-ordered.  d_stats and d_workspace must be 8-byte aligned
 * (d_workspace may be NULL when no bytes are needed).  RT_EINVAL (nothing is
 * launched) for block_len == 0 and everything rt_channel_stats_device
 * refuses. */
int rt_block_stats_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans, size_t block_len,
                          double* d_stats, void* d_workspace, size_t workspace_bytes, void* stream);
/* The resident-block dedispersion call with an optional band table and an
 * optional block mask: d_bands NULL with nbands == 0 is
 * rt_dedisperse_device_opt, a table rt_dedisperse_bands_device; bm NULL is
 * that call itself (the same kernels), a mask (cells and fill in device
 * memory) gives the bits of that call on a block holding x'.  RT_EINVAL
 * (nothing is launched) for a mask refused as above, a misaligned fill, and
 * everything those calls refuse. */
int rt_dedisperse_device_cells(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, const uint8_t* d_mask, size_t ndm, const uint32_t* d_bands,
                               size_t nbands, int64_t max_delay, float* d_out, size_t out_stride, size_t out_offset,
                               void* d_workspace, size_t workspace_bytes, void* stream, uint32_t flags,
                               const rt_block_mask* bm);
/* rt_zero_dm_mean_device with an optional block mask: the mean series of x',
 * the bits of the plain call on a block holding x'. */
int rt_zero_dm_mean_device_cells(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                                 const uint8_t* d_mask, float* d_m, void* stream, const rt_block_mask* bm);

/* ---- DM plan: which trials to search, and each one's time decimation */
/* Host only, no device, float64.  freqs_mhz are channel centres, ascending or
 * descending, nchans >= 2.  With
 *   cw     = (max f - min f) / (nchans - 1)          the channel width
 *   flo    = min f - cw / 2,  fhi = max f + cw / 2   the band edges
 *   fmid   = (flo + fhi) / 2
 *   kdisp  = kdm * (1 / flo^2 - 1 / fhi^2)
 *   ksmear = kdm * (1 / (fmid - cw/2)^2 - 1 / (fmid + cw/2)^2)
 *   s(DM)  = max(wmin, ksmear * DM)                  the smearing at that DM
 *   r(DM)  = s(DM) / kdisp                           the coverage radius
 * the trials are DM_0 = dm_min and DM_{i+1} the DM whose radius touches the
 * previous one's, DM_{i+1} - r(DM_{i+1}) = DM_i + r(DM_i): with e = DM_i +
 * r(DM_i), e + wmin / kdisp, or when ksmear times that exceeds wmin,
 * e / (1 - ksmear / kdisp).  The last trial is the first with DM + r(DM) >=
 * dm_max.  downsamp[i] is the largest power of two f <= max_downsamp with
 * f * tsamp * oversample <= s(DM_i), at least 1; it never decreases with i.
 * *ntrials is the number of trials; dms and downsamp (both or neither NULL:
 * a count alone) take them when capacity >= *ntrials.  RT_EINVAL for nchans <
 * 2, a frequency, tsamp, wmin, oversample or kdm that is not positive and
 * finite, a dm_min that is negative or not finite, dm_max < dm_min or not
 * finite, max_downsamp outside [1, RT_DEDISP_MAX_DOWNSAMP], more than
 * RT_DM_PLAN_MAX_TRIALS trials, or a capacity below the count. */
#define RT_DEDISP_MAX_DOWNSAMP 256
#define RT_DM_PLAN_MAX_TRIALS (1u << 20)
int rt_dm_plan(const double* freqs_mhz, size_t nchans, double tsamp, double dm_min, double dm_max, double wmin,
               double oversample, uint32_t max_downsamp, double kdm, double* dms, uint32_t* downsamp,
               size_t capacity, size_t* ntrials);

/* ---- dedispersion decimated in time: a step of factor f */
/* Decimation first, the sum second.  With x' the block after the block mask
 * (under RT_DEDISP_ZERO_DM: x' - m, as above), f = downsamp and delays the
 * table of rt_dedisperse_delays at tsamp * f:
 *   z[u, c]   = sum over i = 0 .. f - 1 of x'[f * u + i, c]     u < nsamp / f
 *   out[d, u] = sum over unmasked c, ascending, of z[u + delay[d, c], c]
 * Both sums are float32 additions from 0.0f in index order.  For 8-bit and
 * 1/2/4-bit samples without the zero-DM filter every partial sum is an
 * integer: a call with vmax * f * nchans >= 2^24 (vmax = 255, or 2^nbits - 1)
 * is RT_EINVAL, so those outputs are exact.  The trailing nsamp % f samples
 * are dropped.  f = 1 is rt_dedisperse_host_opt, bit for bit. */
/* Host only, no device: the specification.  delays int64 [ndm, nchans] in
 * decimated samples, every entry in [0, max_delay]; out [ndm, nout] with nout
 * + max_delay <= nsamp / f; bm NULL or a block mask in host memory whose
 * t_origin is a multiple of f.  RT_EINVAL for downsamp outside [1,
 * RT_DEDISP_MAX_DOWNSAMP], the exactness cap, and everything
 * rt_dedisperse_host_opt and rt_block_replace_host refuse. */
int rt_dedisperse_ds_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                          const uint8_t* mask, size_t ndm, int64_t max_delay, size_t downsamp, size_t nout,
                          float* out, uint32_t flags, const rt_block_mask* bm);
/* One step of a step table: ndm DMs of one factor.  The step's delay table is
 * int32 [ndm, nchans] from element delays_off of the call's delay array, its
 * output rows start at float out_off of the call's output array:
 *   out[out_off + d * out_stride + out_offset + u]
 * for u in [0, nsamp_blk / downsamp - max_delay). */
typedef struct rt_dedisp_step {
    uint64_t delays_off;   /* int32 elements into d_delays */
    uint64_t out_off;      /* floats into d_out */
    uint64_t out_stride;   /* floats between DM rows */
    uint64_t out_offset;   /* first column written */
    uint32_t ndm;          /* >= 1 */
    uint32_t max_delay;    /* decimated samples */
    uint32_t downsamp;     /* f, in [1, RT_DEDISP_MAX_DOWNSAMP] */
    uint32_t reserved;     /* 0 */
} rt_dedisp_step;
/* Host only, no device: the checks of rt_dedisperse_steps_device on a step
 * table in host memory.  RT_EINVAL for nsteps == 0 or a NULL table, a
 * downsamp outside [1, RT_DEDISP_MAX_DOWNSAMP], ndm == 0 or too many DMs,
 * max_delay >= nsamp_blk / downsamp, a non-zero reserved, the exactness cap
 * above, a delay table that leaves the delays_len elements, output rows that
 * leave the out_floats floats or an out_stride below out_offset plus the
 * step's outputs, a block mask whose t_origin is not a multiple of every
 * downsamp, and the shapes rt_dedisperse_device_cells refuses. */
int rt_dedisperse_steps_check(int dtype, size_t nsamp_blk, size_t nchans, const rt_dedisp_step* steps,
                              size_t nsteps, size_t delays_len, size_t out_floats, uint32_t flags,
                              const rt_block_mask* bm);
/* Device workspace bytes of rt_dedisperse_steps_device: the rows of
 * rt_dedisperse_workspace_bytes_opt, then one float32 area of nchans rows of
 * nsamp_blk / f samples (the pitch padded to 16 bytes) for the smallest f > 1
 * of factors[nfactors], which every decimated step reuses in stream order. */
int rt_dedisperse_steps_workspace_bytes(int dtype, size_t nsamp_blk, size_t nchans, const uint32_t* factors,
                                        size_t nfactors, uint32_t flags, size_t* bytes);
/* Every step of a table from one resident block, stream-ordered, no
 * synchronisation: the block goes to the channel-major rows once, as in
 * rt_dedisperse_device_cells; a step with downsamp == 1 is that call's sum
 * (its bits), any other first decimates the rows into the float32 area and
 * sums those with the float32 sum.  steps is in host memory.  RT_EINVAL
 * (nothing is launched) for everything rt_dedisperse_steps_check refuses, a
 * NULL or misaligned pointer and a workspace below
 * rt_dedisperse_steps_workspace_bytes. */
int rt_dedisperse_steps_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                               const int32_t* d_delays, size_t delays_len, const uint8_t* d_mask,
                               const rt_dedisp_step* steps, size_t nsteps, float* d_out, size_t out_floats,
                               void* d_workspace, size_t workspace_bytes, void* stream, uint32_t flags,
                               const rt_block_mask* bm);
/* Host-buffer form, as rt_dedisperse_opt: x, the delays (int64 [delays_len],
 * every step's entries in [0, its max_delay]) and the mask are uploaded, out
 * [out_floats] copied back.  Synchronous; no block mask. */
int rt_dedisperse_steps(const void* x, int dtype, size_t nsamp, size_t nchans, const int64_t* delays,
                        size_t delays_len, const uint8_t* mask, const rt_dedisp_step* steps, size_t nsteps,
                        float* out, size_t out_floats, uint32_t flags);

/* ------------------------------ pulse cutouts ------------------------------ */
/* Dedispersed, time-decimated windows of one block, one per job: the
 * frequency-time and DM-time cutouts of single-pulse candidates.  Let x' be
 * the block [nsamp, nchans] of any sample type above after the block mask (bm
 * with its t_origin; NULL: none), and under RT_DEDISP_ZERO_DM y = x' - m with
 * m the mean series over the unmasked channels (rt_zero_dm_mean_host of x').
 * delays is int32 [ndelay_rows, nchans]; an entry is clamped to [0, max_delay]
 * as it is read.  Job (start, factor f, nbins T, delay_row, [band_lo,
 * band_hi), out_off) writes
 *   out[out_off + n] = sum over unmasked c in [band_lo, band_hi), ascending,
 *                      sum over j = 0 .. f - 1, ascending, of
 *                      x'[start + n * f + j + delays[delay_row][c], c]
 * for n = 0 .. T - 1.  start is relative to row 0 of the block and may be
 * negative.  A sample whose row is outside [0, nsamp) is skipped: not added
 * and not counted.  An empty band, or one whose channels are all masked,
 * gives zeros.  The ranges [out_off, out_off + nbins) of the jobs of a call
 * must not overlap.
 * Exactness: the 8-bit types (U8, I8, U1, U2, U4) without the zero-DM filter
 * are summed as integers (an int8 sample as its signed value) and converted
 * to float32 once; F32, U16 and everything under RT_DEDISP_ZERO_DM use one
 * float32 accumulator from 0.0f, a round-to-nearest addition per sample in
 * exactly the order above.  The device call returns the host call's bits for
 * every type.
 * RT_EINVAL (device: nothing is launched) for an unknown type or flag, nchans,
 * nsamp or ndelay_rows of 0, nsamp >= 2^31, max_delay outside [0, 2^31), more
 * than RT_DEDISP_MAX_CHANS_8BIT channels of an 8-bit type, a mask refused as
 * above, and a job with factor or nbins of 0, nbins * factor >= 2^31, start
 * outside [-2^40, 2^40], delay_row >= ndelay_rows, a band that is not lo <=
 * hi <= nchans, (band_hi - band_lo) * factor * 255 >= 2^31 where the sum is
 * an integer one, or out_off + nbins > out_floats. */
typedef struct rt_cutout_spec {
    int64_t  start;      /* first sample of bin 0 at delay 0, relative to the block */
    uint64_t out_off;    /* float offset of bin 0 in out */
    uint32_t factor;     /* samples summed per bin, >= 1 */
    uint32_t nbins;      /* >= 1 */
    uint32_t delay_row;  /* row of the delay table */
    uint32_t band_lo;    /* channels [band_lo, band_hi) */
    uint32_t band_hi;
    uint32_t reserved;   /* 0 */
} rt_cutout_spec;
/* Host only, no device: the specification.  Every array is in host memory. */
int rt_pulse_cutouts_host(const void* x, int dtype, size_t nsamp, size_t nchans, const int32_t* delays,
                          size_t ndelay_rows, int64_t max_delay, const uint8_t* mask, const rt_cutout_spec* jobs,
                          size_t njobs, float* out, size_t out_floats, uint32_t flags, const rt_block_mask* bm);
/* One resident block, stream-ordered, no synchronisation: the block goes to
 * the channel-major rows of the dedispersion workspace (d_workspace of
 * rt_dedisperse_workspace_bytes_opt(dtype, nsamp_blk, nchans, flags) bytes,
 * 16-byte aligned), as the first step of rt_dedisperse_device_cells, then one
 * launch for all jobs.  jobs is in host memory and is checked there; d_jobs is
 * device memory for njobs rt_cutout_spec, 8-byte aligned, which the call
 * fills.  d_delays, d_mask, d_out (out_floats floats, 4-byte aligned) and the
 * mask's cells and fill are device memory.  njobs == 0 launches nothing. */
int rt_pulse_cutouts_device(const void* d_block, int dtype, size_t nsamp_blk, size_t nchans,
                            const int32_t* d_delays, size_t ndelay_rows, int64_t max_delay, const uint8_t* d_mask,
                            const rt_cutout_spec* jobs, size_t njobs, rt_cutout_spec* d_jobs, float* d_out,
                            size_t out_floats, void* d_workspace, size_t workspace_bytes, void* stream,
                            uint32_t flags, const rt_block_mask* bm);
/* The kernel's shape, for tests to name the path they run (no device call):
 * the bins of a tile, and for a channel whose clamped span of a tile is the
 * elements [lo, hi) of its row (esize 1: 8-bit rows, 4: float rows) the dwords
 * it takes and whether they go through LDS (staged) or the row is read
 * directly.  Both paths give the same bits. */
int rt_pulse_cutouts_plan(size_t esize, int64_t lo, int64_t hi, size_t* tile, size_t* ndw, int* staged);

/* ---------------------------- signal injection ----------------------------- */
/* Synthetic pulsars and single pulses added, in place, to a time-major block
 * x[nsamp][nchans] of RT_DEDISP_U8, RT_DEDISP_I8 or RT_DEDISP_F32 samples
 * (contiguous rows) whose row 0 is absolute sample t_origin of the
 * observation.  The packed types are refused.  K signals, one rt_inject_spec
 * each, name their arrays by offsets into three packed arrays: tmpl (float32),
 * amp (float32, nchans per signal) and delay (int32, nchans per signal, the
 * table of rt_dedisperse_delays at the signal's DM).
 *
 * For absolute sample t = t_origin + row, channel c and signal k -- 64-bit
 * two's-complement integers that wrap, unless said otherwise:
 *   u    = t - delay[k][c]
 *   s    = 0 when factor == 0, otherwise
 *          (int64) rint(factor * (double)(u * ((int64)span - u)))
 *          (int64 -> double rounds to nearest even; one IEEE multiply;
 *          rint rounds half to even)
 *   ue   = u + s
 *   kind 0:  ph  = phase0 + (uint64)ue * step                    (mod 2^64)
 *            v_k = amp[k][c] * tmpl[k][ph >> (64 - log2bins)]
 *   kind 1:  i   = ue - t0
 *            v_k = amp[k][c] * tmpl[k][i] when 0 <= i < length, otherwise 0.0f
 * v_k is a float32 product, rounded before any addition; acc = (((0.0f + v_0)
 * + v_1) + ...) in signal order, float32 additions.  Then
 *   F32:      x = x + acc
 *   U8 / I8:  x = clamp(x + (int32) floorf(clampf(acc + r)), lo, hi)
 * with clampf(v) = fminf(fmaxf(v, -65536.0f), 65536.0f) (a NaN becomes
 * -65536), [lo, hi] the type's range and the dither
 *   r = (float)(z >> 40) * 2^-24, z = mix(t * nchans + c + seed * 0x9E3779B97F4A7C15)
 *   mix: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *        z *= 0x94D049BB133111EB; z ^= z >> 31        (the splitmix64 finaliser)
 * a stochastic rounding that is unbiased, reproducible, and a function of the
 * absolute sample alone: the result does not depend on how an observation is
 * cut into blocks.  With K == 0 nothing is touched; where acc == 0 a sample is
 * unchanged.  Host and device results have the same bits.
 *
 * step = round(2^64 * tsamp / P) and phase0 count 2^-64 turns.  factor is the
 * f of the resampling above (accel * tsamp / (2 c)) and span its N: u + s is
 * the first-order inverse of out[j] = x[j - s_j], so the search's resampling
 * at the same f maps the injected train back to a periodic one up to the
 * residual s_j - s_(j - s_j), the change of s over a distance of |s| samples:
 * at most (|f| * span)^2 * span / 4 + 1 samples, since |ds/dj| <= |f| * span
 * and |s| <= |f| * span^2 / 4.  The inverse is first
 * order, not exact.  One template per signal: no per-channel smearing.
 *
 * RT_EINVAL (nothing is written or launched) for a sample type other than the
 * three, nchans above RT_INJECT_MAX_CHANS, t_origin + nsamp >= 2^31, and for a
 * signal with: a kind other than 0 or 1, kind 0 with log2bins outside [1, 16],
 * kind 1 with length == 0, span above RT_RESAMPLE_MAX_SAMPLES, a factor that
 * is not finite, has fabs(factor) * (double)span >= 1.0 or is not zero while
 * span is, a non-zero reserved, a template, amplitude or delay range that runs
 * past its array, or -- where the arrays are host memory -- an amplitude or a
 * template value that is not finite. */
#define RT_INJECT_MAX_CHANS 16777216
typedef struct rt_inject_spec {
    uint64_t tmpl_off;   /* float offset of the template in tmpl: 2^log2bins (kind 0) or length (kind 1) entries */
    uint64_t amp_off;    /* float offset of the nchans amplitudes in amp */
    uint64_t delay_off;  /* int32 offset of the nchans delays in delay */
    uint64_t step;       /* kind 0: phase per sample, 2^-64 turns */
    uint64_t phase0;     /* kind 0: phase at ue = 0 */
    int64_t  t0;         /* kind 1: the sample of template entry 0 at zero delay */
    double   factor;     /* f of the acceleration map; 0: none */
    uint64_t span;       /* N of the acceleration map */
    uint32_t kind;       /* 0 periodic, 1 single pulse */
    uint32_t log2bins;   /* kind 0: 1 .. 16 */
    uint32_t length;     /* kind 1: >= 1 */
    uint32_t reserved;   /* 0 */
} rt_inject_spec;
/* Host only, no device: every check above on arrays in host memory. */
int rt_inject_check(int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, const rt_inject_spec* specs,
                    size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp, size_t amp_len,
                    const int32_t* delay, size_t delay_len);
/* Host only, no device: the specification, sequential, in place on x. */
int rt_inject_host(void* x, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
                   const rt_inject_spec* specs, size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp,
                   size_t amp_len, const int32_t* delay, size_t delay_len);
/* The same, in place on a device-resident block (any byte alignment for the
 * 8-bit types, 4 bytes for F32).  Stream-ordered: one launch, no host
 * synchronisation, no device allocation and no workspace.  specs is host
 * memory and is checked there; d_specs is the same table in device memory
 * (8-byte aligned), d_tmpl, d_amp and d_delay the packed arrays in device
 * memory, which the caller uploads once for as many blocks as it likes and
 * whose values it has put through rt_inject_check. */
int rt_inject_device(void* d_block, int dtype, size_t nsamp_blk, size_t nchans, uint64_t t_origin, uint64_t seed,
                     const rt_inject_spec* specs, size_t nspecs, const rt_inject_spec* d_specs, const float* d_tmpl,
                     size_t tmpl_len, const float* d_amp, size_t amp_len, const int32_t* d_delay, size_t delay_len,
                     void* stream);
/* Host-buffer form: rt_inject_check, then the block and the tables are
 * uploaded, rt_inject_device runs and the block is copied back.  Synchronous. */
int rt_inject(void* x, int dtype, size_t nsamp, size_t nchans, uint64_t t_origin, uint64_t seed,
              const rt_inject_spec* specs, size_t nspecs, const float* tmpl, size_t tmpl_len, const float* amp,
              size_t amp_len, const int32_t* delay, size_t delay_len);

/* --------------------------- file input (device) --------------------------- */
/* 8-bit SIGPROC samples (riptide/time_series.py:352-357) to float32 in device
 * memory: d_raw holds n bytes, int8 when is_signed else uint8; exact as
 * numpy's astype(np.float32).  d_raw must be 4-byte aligned. */
int rt_convert_samples_device(const void* d_raw, size_t n, int is_signed, float* d_out, void* stream);

/* ----------------------------- profiling ---------------------------------- */
/* When enabled, rt_periodogram_device records HIP events around every cone
 * (FFA pass) launch and accumulates their time and algorithmic bytes
 * (4mp read + 4mp or 4*rows_eval*W written per pass). */
int rt_profile_enable(int on);
/* kind: 0 = FFA cone passes, 1 = downsample ladder.  Synchronises the events. */
int rt_profile_read(int kind, double* milliseconds, double* alg_bytes, double* moved_bytes, uint64_t* launches);
int rt_profile_reset(void);

/* Diagnostics (meaningful in the -DRT_STAMPS build, libriptide_amd_stamps.so):
 * cone-kernel cycles per phase summed over work items -- [0] prologue,
 * [1] bottom-level fill, [2] row descriptors, [3] merge levels, [4] store,
 * [5] fused S/N, [7] items.  The first call allocates the counters. */
int rt_diag_stamps(uint64_t* out8, int reset);
/* Diagnostic builds: per-unit timeline records (8 words each: hw id | xcc << 32,
 * start, setup done, fill landed, merge done, end, unit, shape), up to cap. */
int rt_diag_timeline(uint64_t* out, uint64_t cap, uint64_t* count);
/* Diagnostic builds: index of each cone launch's first timeline record (one
 * entry per launch since the last rt_diag_stamps reset), up to cap. */
int rt_diag_launches(uint64_t* out, uint64_t cap, uint64_t* count);

/* Plan statistics: transforms, work items, passes, cone launches per trial. */
int rt_plan_stats(const rt_plan* plan, uint64_t* transforms, uint64_t* items, uint64_t* launches,
                  double* alg_bytes_per_trial, double* moved_bytes_per_trial, uint64_t* cells_per_trial);


#ifdef __cplusplus
}
#endif

#endif /* RIPTIDE_AMD_H */
