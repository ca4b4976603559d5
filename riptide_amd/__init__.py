"""riptide_amd: MI355X-native FFA periodogram engine with riptide's Python API.

The compute path (downsampling ladder, FFA transform, boxcar S/N, running
median dereddening, normalisation) runs in hand-written HIP kernels for gfx950
behind the C ABI in include/riptide_amd.h; ``riptide_amd.libcpp`` is a drop-in
for riptide's ``riptide.libcpp`` module.
"""
__version__ = "0.1.0"

from .clustering import cluster1d
from .ffautils import generate_width_trials
from .metadata import Metadata
from .peak_detection import Peak, find_peaks
from .periodogram import Periodogram

# Compute API: needs the engine library (raises ImportError if it was not built)
from .libffa import boxcar_snr, downsample, ffa1, ffa2, ffafreq, ffaprd, generate_signal
from .running_medians import fast_running_median, running_median
from .search import ffa_search
from .time_series import TimeSeries
from .peak_cluster import PeakCluster
from .candidate import Candidate, build_candidates, build_candidates_filterbank
from .harmonic_testing import apply_candidate_filters, flag_harmonics, hdiag, htest
from .reading import Filterbank, PackedFilterbank, open_filterbank
from .dispatch import search_filterbank, search_filterbank_accel, search_filterbank_plan
from .dedispersion import DMPlan, dm_plan
from .refine import Refinement, refine_candidates, refine_cube
from .single_pulse import SinglePulse, search_filterbank_pulses
from .pulse_candidates import PulseCandidate, build_pulse_candidates
from .injection import InjectionTables, PulsarSignal, PulseSignal, inject_filterbank, injection_tables
from . import acceleration, dedispersion, injection, pulse_candidates, rfi, single_pulse

__all__ = [
    "Candidate", "PeakCluster", "build_candidates", "build_candidates_filterbank", "flag_harmonics",
    "apply_candidate_filters", "htest", "hdiag",
    "TimeSeries", "Periodogram", "Metadata", "ffa_search", "ffa1", "ffa2", "ffafreq", "ffaprd",
    "generate_signal", "downsample", "boxcar_snr", "find_peaks", "running_median",
    "fast_running_median", "generate_width_trials", "cluster1d", "Peak", "Filterbank", "search_filterbank",
    "PackedFilterbank", "open_filterbank",
    "dedispersion", "rfi", "Refinement", "refine_cube", "refine_candidates",
    "SinglePulse", "search_filterbank_pulses", "single_pulse",
    "PulseCandidate", "build_pulse_candidates", "pulse_candidates",
    "acceleration", "search_filterbank_accel",
    "dm_plan", "DMPlan", "search_filterbank_plan",
    "injection", "PulsarSignal", "PulseSignal", "InjectionTables", "injection_tables", "inject_filterbank",
]
