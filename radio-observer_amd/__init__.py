"""radio-observer_amd -- MI355X-native STFT / waterfall / bolid-scan hot path.

Layout:
  csrc/      hand-written gfx950 kernels + the C ABI (include/ro_stft.h)
  capi.py    ctypes binding of that C ABI (plumbing for tests / bench)
  build.py   in-tree hipcc build of libro_stft.so

The directory name follows the reference repo (`radio-observer`), so import it
with importlib:  ro = importlib.import_module("radio-observer_amd").
There is no CPU fallback: without libro_stft.so / a gfx950 device the compute
entry points raise.
"""
from . import build as _build  # noqa: F401
from . import capi  # noqa: F401
from .capi import (  # noqa: F401
    Stft, StftError, Bands, BandWindow, ScanRecord, PinnedArray, library, library_path, hip_runtimes, require_one_hip_runtime,
    clamp_overlap, fft_sample_rate, frequency_to_bin, bin_to_frequency, time_to_fft_samples,
    row_count, window_table, bins_supported, device_count, shard_rows, shard_samples, shard_max_rows,
    stitch_rows, ln_levels, band_supported, bands_hull, band_windows_supported, bands_windows,
    tile_windows_supported, merge_windows, events_host, Detector,
    EVENT_DTYPE, DETECT_STATE_DTYPE, DETECT_SUMMARY_DTYPE,
    snapshots_host, RowRing, ROW_RING, SNAPSHOT_DTYPE, SNAP_SUMMARY_DTYPE, RO_SNAP_CAPTURED, RO_SNAP_EMPTY, RO_SNAP_LOST,
    raw_host, IqSpan, RAW_CAPTURE_DTYPE, RAW_SUMMARY_DTYPE, RO_MAX_IQ_SPANS,
    snapshot_units_host, raw_units_host, FITS_UNIT_DTYPE, UNIT_SUMMARY_DTYPE, RO_FITS_BLOCK,
    RO_UNIT_WRITTEN, RO_UNIT_SKIPPED, RO_UNIT_NO_ROOM, RO_UNIT_INVALID,
    snapshot_rows, periodic_plan, periodic_units_host, periodic_recorders, PERIODIC_DTYPE, PERIODIC_ENTRY_DTYPE,
    PERIODIC_SUMMARY_DTYPE, RO_MAX_PERIODIC, RO_PERIODIC_WRITTEN, RO_PERIODIC_LOST, RO_PERIODIC_NO_ROOM,
    snapshot_levels_host, periodic_levels_host, LEVEL_RANGE_DTYPE, RO_LEVEL_BLOCK,
    png_bytes, levels_png_host, levels_png_deflate_host, periodic_level_dir, RO_PNG_ALIGN,
    resize_shape, resize_plan, levels_resize_host, RESIZE_INFO_DTYPE,
    RO_WINDOW_NUTTALL, RO_WINDOW_HANN, RO_WINDOW_CUSTOM, RO_IQ_F32, RO_IQ_I16, RO_IQ_F64,
    RO_PRECISION_F32, RO_PRECISION_F64,
)

def sharding():
    """time-chunk sharding helpers (radio-observer_amd/timeshard.py; imports torch lazily)"""
    import importlib
    return importlib.import_module(__name__ + ".timeshard")


__all__ = ["capi", "Stft", "StftError", "Bands", "ScanRecord", "library"]
