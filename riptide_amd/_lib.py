"""ctypes loader of the engine's C ABI (include/riptide_amd.h).

The shared library is built in-tree (``make -C riptide_amd/csrc``, or
``__graft_entry__.build()``) and loaded from this package directory.  There is
no fallback: if the library is missing or fails to load, importing the compute
API raises, loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RIPTIDE_AMD_LIB") or os.path.join(_HERE, "libriptide_amd.so")

RT_OK, RT_EINVAL, RT_EHIP, RT_EINTERNAL = 0, 1, 2, 3

_c_sz = ctypes.c_size_t
_c_d = ctypes.c_double
_c_f = ctypes.c_float
_c_i = ctypes.c_int
_vp = ctypes.c_void_p
_psz = ctypes.POINTER(ctypes.c_size_t)
_pd = ctypes.POINTER(ctypes.c_double)
_pu64 = ctypes.POINTER(ctypes.c_uint64)

# name -> (restype, argtypes); pointers are passed as c_void_p (numpy .ctypes.data
# or torch .data_ptr())
_SIGNATURES = {
    "rt_last_error": (ctypes.c_char_p, []),
    "rt_version": (ctypes.c_char_p, []),
    "rt_set_device": (_c_i, [_c_i]),
    "rt_rollback": (_c_i, [_vp, _c_sz, _c_sz, _vp]),
    "rt_fused_rollback_add": (_c_i, [_vp, _vp, _c_sz, _c_sz, _vp]),
    "rt_circular_prefix_sum": (_c_i, [_vp, _c_sz, _c_sz, _vp]),
    "rt_ffa2": (_c_i, [_vp, _c_sz, _c_sz, _vp]),
    "rt_benchmark_ffa2": (_c_i, [_c_sz, _c_sz, _c_sz, _pd]),
    "rt_snr1": (_c_i, [_vp, _c_sz, _vp, _c_sz, _c_f, _vp]),
    "rt_snr2": (_c_i, [_vp, _c_sz, _c_sz, _vp, _c_sz, _c_f, _vp]),
    "rt_downsampled_size": (_c_sz, [_c_sz, _c_d]),
    "rt_downsample": (_c_i, [_vp, _c_sz, _c_d, _vp]),
    "rt_downsample_rows": (_c_i, [_vp, _c_sz, _c_sz, _c_d, _vp]),
    "rt_fold_shape": (_c_i, [_c_sz, _c_d, _c_sz, _c_sz, _psz, _psz]),
    "rt_fold_workspace_bytes": (_c_i, [_c_sz, _vp, _c_sz, _psz]),
    "rt_fold_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp]),
    "rt_fold": (_c_i, [_vp, _c_sz, _c_sz, _vp, _c_sz, _vp, _c_sz]),
    # period, span, bins, subints, band freqs, bands, dm, kdm, periods, nper, dms, ndm, pshift, dshift
    "rt_refine_shifts": (_c_i, [_c_d, _c_d, _c_sz, _c_sz, _vp, _c_sz, _c_d, _c_d, _vp, _c_sz, _vp, _c_sz, _vp, _vp]),
    # cube, bands, subints, bins, dshift, ndm, pshift, nper, widths (uint32), nw, stdnoise, snr, prof or NULL
    "rt_refine_host": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp, _c_sz, _c_f, _vp, _vp]),
    "rt_refine_workspace_bytes": (_c_i, [_vp, _c_sz, _psz]),
    # cubes, shifts, widths, specs, nspecs, snr, profiles or NULL, workspace, workspace bytes, stream
    "rt_refine_device": (_c_i, [_vp, _vp, _vp, _vp, _c_sz, _vp, _vp, _vp, _c_sz, _vp]),
    "rt_refine": (_c_i, [_vp, _vp, _vp, _vp, _c_sz, _vp, _vp]),
    # x, nseries, size, ldx, widths (int32, host), nw, threshold, radius, events, capacity, count (uint64), best,
    # kbest
    "rt_single_pulse_host": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _c_f, _c_sz, _vp, _c_sz, _vp, _vp, _vp]),
    "rt_single_pulse_limits": (_c_i, [_psz, _psz]),
    # wmax, radius, chunk, chunk_segs, lds_bytes
    "rt_single_pulse_plan": (_c_i, [_c_sz, _c_sz, _psz, _psz, _psz]),
    # nseries, size, nw, capacity, bytes
    "rt_single_pulse_workspace_bytes": (_c_i, [_c_sz, _c_sz, _c_sz, _c_sz, _psz]),
    # as the host form with device x, events, count, best, kbest; then workspace, workspace bytes, stream
    "rt_single_pulse_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _c_f, _c_sz, _vp, _c_sz, _vp, _vp, _vp,
                                      _vp, _c_sz, _vp]),
    # x, nseries, size, ldx, src (int32, host), factor (float64, host), nrows, out, ldo
    "rt_resample_host": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz]),
    # the same with device x and out; then stream
    "rt_resample_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, _vp]),
    "rt_periodogram_length": (_c_i,[_c_sz, _c_d, _c_d, _c_d, _c_sz, _c_sz, _psz]),
    "rt_periodogram": (_c_i, [_vp, _c_sz, _c_d, _vp, _c_sz, _c_d, _c_d, _c_sz, _c_sz, _vp, _vp, _vp]),
    "rt_running_median": (_c_i, [_vp, _c_sz, _c_sz, _vp]),
    "rt_fast_running_median": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _vp]),
    "rt_deredden_normalise": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _c_i, _c_i, _vp]),
    "rt_periodogram_grid": (_c_i, [_c_sz, _c_d, _c_d, _c_d, _c_sz, _c_sz, _vp, _vp]),
    "rt_ffa_schedule_check": (_c_i, [_c_sz, _c_sz, _pu64]),
    "rt_schedule_check": (_c_i, [_c_sz, _c_d, _c_sz, _c_d, _c_d, _c_sz, _c_sz, _pu64, _pu64, _pu64, _pd, _pd,
                                 _pu64]),
    # size, tsamp, num_widths, pmin, pmax, bmin, bmax, items (rt_schedule_item[cap]), cap, count
    "rt_schedule_items": (_c_i, [_c_sz, _c_d, _c_sz, _c_d, _c_d, _c_sz, _c_sz, _vp, _c_sz, _pu64]),
    "rt_schedule_final_kinds": (_c_i, [_c_sz, _c_d, _vp, _c_sz, _c_d, _c_d, _c_sz, _c_sz, _pu64, _pu64, _pu64, _vp,
                                       _c_sz]),
    "rt_plan_create": (_c_i, [_c_sz, _c_d, _vp, _c_sz, _c_d, _c_d, _c_sz, _c_sz, _vp]),
    "rt_plan_destroy": (None, [_vp]),
    "rt_plan_shape": (_c_i, [_vp, _psz, _psz]),
    "rt_plan_grid": (_c_i, [_vp, _vp, _vp]),
    "rt_plan_workspace_bytes": (_c_i, [_vp, _c_sz, _psz]),
    "rt_periodogram_device": (_c_i, [_vp, _vp, _c_sz, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp]),
    "rt_periodogram_ladder_device": (_c_i, [_vp, _vp, _c_sz, _c_sz, _vp, _c_sz, _vp]),
    "rt_periodogram_passes_device": (_c_i, [_vp, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp]),
    "rt_plan_check": (_c_i, [_vp, _vp]),
    "rt_deredden_workspace_bytes": (_c_i, [_c_sz, _c_sz, _c_sz, _c_sz, _psz]),
    # size, width, min_points, deredden, normalise, in / out address mod 16, in / out stride, rt_dered_forms*
    "rt_deredden_forms": (_c_i, [_c_sz, _c_sz, _c_sz, _c_i, _c_i, ctypes.c_uint, ctypes.c_uint, _c_sz, _c_sz, _vp]),
    "rt_deredden_normalise_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_i, _c_i, _vp, _c_sz,
                                            _vp, _c_sz, _vp]),
    "rt_profile_enable": (_c_i, [_c_i]),
    "rt_profile_read": (_c_i, [_c_i, _pd, _pd, _pd, _pu64]),
    "rt_profile_reset": (_c_i, []),
    "rt_diag_stamps": (_c_i, [_pu64, _c_i]),
    "rt_diag_timeline": (_c_i, [_pu64, ctypes.c_uint64, _pu64]),
    "rt_diag_launches": (_c_i, [_pu64, ctypes.c_uint64, _pu64]),
    "rt_plan_stats": (_c_i, [_vp, _pu64, _pu64, _pu64, _pd, _pd, _pu64]),
    "rt_convert_samples_device": (_c_i, [_vp, _c_sz, _c_i, _vp, _vp]),
    "rt_segment_order_stats_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _c_sz, _vp, _vp]),
    "rt_threshold_select_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _c_d, _vp, _vp, _c_sz,
                                          _vp]),
    "rt_find_peaks_workspace_bytes": (_c_i, [_c_sz, _c_sz, _c_sz, _c_sz, _psz]),
    # snrs, batch, stride, L, W, logf, freqs, coeffs, ncoef, smin, radius, counts, rows, snr, cap, chunk_rows,
    # workspace, workspace bytes, stream
    "rt_find_peaks_device": (_c_i, [_vp, _c_sz, _c_sz, _c_sz, _c_sz, _vp, _vp, _vp, _c_sz, _c_d, _c_d, _vp, _vp, _vp,
                                    _c_sz, _c_sz, _vp, _c_sz, _vp]),
    "rt_find_peaks_host": (_c_i, [_vp, _c_sz, _c_sz, _vp, _vp, _vp, _c_sz, _c_d, _c_d, _vp, _vp, _vp, _c_sz]),
    "rt_ladder_check": (_c_i, [_c_sz, _c_d, _c_d, _c_d, _c_sz, _c_sz, ctypes.POINTER(_c_i), _pu64]),
    # the six search parameters, rungs (rt_ladder_rung[cap]), cap, count, leaf_floats, mode, margin
    "rt_ladder_layout": (_c_i, [_c_sz, _c_d, _c_d, _c_d, _c_sz, _c_sz, _vp, _c_sz, _pu64, _pu64,
                                ctypes.POINTER(_c_i), ctypes.POINTER(ctypes.c_uint32)]),
    # freq, snr, ducy, dm, n, pi, pj, npairs, params, num, den, phase, dm, snr distances
    "rt_hdiag_host": (_c_i, [_vp, _vp, _vp, _vp, _c_sz, _vp, _vp, _c_sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_hdiag_pairs": (_c_i, [_vp, _vp, _vp, _vp, _c_sz, _vp, _vp, _c_sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_flag_harmonics": (_c_i, [_vp, _vp, _vp, _vp, _c_sz, _vp, _c_sz, _vp, _vp, _vp]),
    "rt_flag_harmonics_stats": (_c_i, [_pu64, _pu64, _pu64, _pd]),
    # dtype, nchans, bytes
    "rt_dedisp_row_bytes": (_c_i, [_c_i, _c_sz, _psz]),
    # freqs, nchans, dms, ndm, tsamp, kdm, delays (int64), max_delay
    "rt_dedisperse_delays": (_c_i, [_vp, _c_sz, _vp, _c_sz, _c_d, _c_d, _vp, ctypes.POINTER(ctypes.c_int64)]),
    # x, dtype, nsamp, nchans, delays (int64), mask, ndm, max_delay, nout, out
    "rt_dedisperse_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _c_sz, _vp]),
    "rt_dedisperse_workspace_bytes": (_c_i, [_c_i, _c_sz, _c_sz, _psz]),
    # block, dtype, nsamp_blk, nchans, delays (int32), mask, ndm, max_delay, out, out_stride, out_offset,
    # workspace, workspace bytes, stream
    "rt_dedisperse_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _vp, _c_sz, _c_sz,
                                    _vp, _c_sz, _vp]),
    # esize, lo, hi, ndw, staged
    "rt_dedisperse_span_plan": (_c_i, [_c_sz, ctypes.c_int64, ctypes.c_int64, _psz, ctypes.POINTER(_c_i)]),
    # x, dtype, nsamp, nchans, delays (int64), mask, ndm, max_delay, out
    "rt_dedisperse":(_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _vp]),
    # the four above with a trailing flags argument (before `bytes` in the workspace query)
    "rt_dedisperse_host_opt": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _c_sz, _vp,
                                      ctypes.c_uint32]),
    "rt_dedisperse_workspace_bytes_opt": (_c_i, [_c_i, _c_sz, _c_sz, ctypes.c_uint32, _psz]),
    "rt_dedisperse_device_opt": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _vp, _c_sz, _c_sz,
                                        _vp, _c_sz, _vp, ctypes.c_uint32]),
    "rt_dedisperse_opt": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _vp, ctypes.c_uint32]),
    # the band forms: bands (uint32 [nbands, 2]) and nbands behind ndm, flags last
    "rt_dedisperse_bands_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, ctypes.c_int64, _c_sz,
                                        _vp, ctypes.c_uint32]),
    "rt_dedisperse_bands_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, ctypes.c_int64, _vp,
                                          _c_sz, _c_sz, _vp, _c_sz, _vp, ctypes.c_uint32]),
    "rt_dedisperse_bands": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, ctypes.c_int64, _vp,
                                   ctypes.c_uint32]),
    # x, dtype, nsamp, nchans, mask, m
    "rt_zero_dm_mean_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp]),
    # block, dtype, nsamp_blk, nchans, mask, m, stream
    "rt_zero_dm_mean_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _vp]),
    # x, dtype, nsamp, nchans, acc (float64 [2, nchans])
    "rt_channel_stats_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp]),
    "rt_channel_stats_workspace_bytes": (_c_i, [_c_sz, _c_sz, _psz]),
    # block, dtype, nsamp_blk, nchans, acc, workspace, workspace bytes, stream
    "rt_channel_stats_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp]),
    # the block mask: `bm` is a pointer to a BlockMaskStruct (rt_block_mask), or None
    # x, dtype, nsamp, nchans, bm, out
    "rt_block_replace_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp]),
    # x, dtype, nsamp, nchans, block_len, stats (float64 [nblk, 2, nchans])
    "rt_block_stats_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _c_sz, _vp]),
    # nsamp_blk, nchans, block_len, bytes
    "rt_block_stats_workspace_bytes": (_c_i, [_c_sz, _c_sz, _c_sz, _psz]),
    # block, dtype, nsamp_blk, nchans, block_len, stats, workspace, workspace bytes, stream
    "rt_block_stats_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp]),
    # rt_dedisperse_bands_device's arguments (bands None, nbands 0: no table), then bm
    "rt_dedisperse_device_cells": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, ctypes.c_int64, _vp,
                                          _c_sz, _c_sz, _vp, _c_sz, _vp, ctypes.c_uint32, _vp]),
    # rt_zero_dm_mean_device's arguments, then bm
    "rt_zero_dm_mean_device_cells": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _vp, _vp]),
    # freqs, nchans, tsamp, dm_min, dm_max, wmin, oversample, max_downsamp, kdm, dms, downsamp (uint32), capacity,
    # ntrials
    "rt_dm_plan": (_c_i, [_vp, _c_sz, _c_d, _c_d, _c_d, _c_d, _c_d, ctypes.c_uint32, _c_d, _vp, _vp, _c_sz, _psz]),
    # x, dtype, nsamp, nchans, delays (int64), mask, ndm, max_delay, downsamp, nout, out, flags, bm
    "rt_dedisperse_ds_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _vp, _c_sz, ctypes.c_int64, _c_sz, _c_sz, _vp,
                                     ctypes.c_uint32, _vp]),
    # the step table: `steps` is a numpy array of engine.DEDISP_STEP_DTYPE (rt_dedisp_step) in host memory
    # dtype, nsamp_blk, nchans, steps, nsteps, delays_len, out_floats, flags, bm
    "rt_dedisperse_steps_check": (_c_i, [_c_i, _c_sz, _c_sz, _vp, _c_sz, _c_sz, _c_sz, ctypes.c_uint32, _vp]),
    # dtype, nsamp_blk, nchans, factors (uint32), nfactors, flags, bytes
    "rt_dedisperse_steps_workspace_bytes": (_c_i, [_c_i, _c_sz, _c_sz, _vp, _c_sz, ctypes.c_uint32, _psz]),
    # block, dtype, nsamp_blk, nchans, delays (int32), delays_len, mask, steps, nsteps, out, out_floats, workspace,
    # workspace bytes, stream, flags, bm
    "rt_dedisperse_steps_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz, _vp,
                                          _c_sz, _vp, ctypes.c_uint32, _vp]),
    # x, dtype, nsamp, nchans, delays (int64), delays_len, mask, steps, nsteps, out, out_floats, flags
    "rt_dedisperse_steps": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _c_sz, _vp, _vp, _c_sz, _vp, _c_sz,
                                   ctypes.c_uint32]),
    # x, dtype, nsamp, nchans, delays (int32 [rows, nchans]), rows, max_delay, mask, jobs (rt_cutout_spec[njobs]),
    # njobs, out, out floats, flags, bm
    "rt_pulse_cutouts_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _c_sz, ctypes.c_int64, _vp, _vp, _c_sz, _vp, _c_sz,
                                     ctypes.c_uint32, _vp]),
    # the same with a device block, delays, mask and out, and behind njobs the device table the call fills;
    # then workspace, workspace bytes, stream, flags, bm
    "rt_pulse_cutouts_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, _vp, _c_sz, ctypes.c_int64, _vp, _vp, _c_sz, _vp, _vp,
                                       _c_sz, _vp, _c_sz, _vp, ctypes.c_uint32, _vp]),
    # esize, lo, hi, tile, ndw, staged
    "rt_pulse_cutouts_plan": (_c_i, [_c_sz, ctypes.c_int64, ctypes.c_int64, _psz, _psz, ctypes.POINTER(_c_i)]),
    # the injection: `specs` is a numpy array of engine.INJECT_SPEC_DTYPE (rt_inject_spec) in host memory
    # dtype, nsamp, nchans, t_origin, specs, nspecs, tmpl, tmpl_len, amp, amp_len, delay (int32), delay_len
    "rt_inject_check": (_c_i, [_c_i, _c_sz, _c_sz, ctypes.c_uint64, _vp, _c_sz, _vp, _c_sz, _vp, _c_sz, _vp, _c_sz]),
    # x, dtype, nsamp, nchans, t_origin, seed, then as above from specs
    "rt_inject_host": (_c_i, [_vp, _c_i, _c_sz, _c_sz, ctypes.c_uint64, ctypes.c_uint64, _vp, _c_sz, _vp, _c_sz, _vp,
                              _c_sz, _vp, _c_sz]),
    "rt_inject": (_c_i, [_vp, _c_i, _c_sz, _c_sz, ctypes.c_uint64, ctypes.c_uint64, _vp, _c_sz, _vp, _c_sz, _vp,
                         _c_sz, _vp, _c_sz]),
    # block, dtype, nsamp_blk, nchans, t_origin, seed, specs (host), nspecs, then device: specs, tmpl, tmpl_len, amp,
    # amp_len, delay, delay_len; stream
    "rt_inject_device": (_c_i, [_vp, _c_i, _c_sz, _c_sz, ctypes.c_uint64, ctypes.c_uint64, _vp, _c_sz, _vp, _vp,
                                _c_sz, _vp, _c_sz, _vp, _c_sz, _vp]),
}


class BlockMaskStruct(ctypes.Structure):
    """rt_block_mask (include/riptide_amd.h); pass ctypes.byref of one as `bm`."""
    _fields_ = [("cells", _vp), ("nblocks", _c_sz), ("block_len", _c_sz), ("t_origin", ctypes.c_uint64),
                ("fill", _vp)]

EXPORTED = tuple(_SIGNATURES)

# test build only (libriptide_amd_testhooks.so, include/riptide_amd_test.h);
# bound when the loaded library has them
_TEST_SIGNATURES = {
    "rt_test_corrupt_next_plans": (_c_i, [_c_i]),
}
TESTHOOKS_PATH = os.path.join(_HERE, "libriptide_amd_testhooks.so")

_lib = None


class EngineError(RuntimeError):
    """A HIP runtime or internal failure inside the engine."""


def load():
    """Load (once) and return the engine library.  Raises ImportError if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"riptide_amd engine library not found at {LIB_PATH}; build it with "
            "`make -C riptide_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: torch ships its own libamdhip64, and an
    # engine library loaded before torch binds /opt/rocm's instead -- the
    # engine's launches then fail with "no ROCm-capable device is detected"
    # once torch initialises its runtime (`import riptide_amd; import torch`).
    # Importing torch first makes the engine resolve to torch's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # The plan pointer is opaque: rt_plan_create takes an rt_plan** (void*)
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in _TEST_SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    """Map an RT_* return code to the reference's exception types."""
    if rc == RT_OK:
        return
    msg = _lib.rt_last_error().decode("utf-8", "replace")
    if rc == RT_EINVAL:
        raise ValueError(msg)
    raise EngineError(msg)


def ptr(a):
    """Raw address of a numpy array or torch tensor."""
    if hasattr(a, "data_ptr"):
        return ctypes.c_void_p(a.data_ptr())
    return ctypes.c_void_p(a.ctypes.data)
