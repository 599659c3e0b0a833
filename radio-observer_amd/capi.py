"""ctypes binding of include/ro_stft.h (the C ABI of libro_stft.so).

Only plumbing lives here: argument marshalling, error-code -> exception.  The
arithmetic is in the HIP kernels.  Device buffers are passed as raw integer
addresses (e.g. torch.Tensor.data_ptr()).
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

RO_WINDOW_NUTTALL, RO_WINDOW_HANN, RO_WINDOW_CUSTOM = 0, 1, 2
RO_IQ_F32, RO_IQ_I16, RO_IQ_F64 = 0, 1, 2
RO_PRECISION_F32, RO_PRECISION_F64 = 0, 1
RO_MAX_EXTRA_BANDS = 7
RO_MAX_BAND_WINDOWS = 8
RO_MAX_TILE_WINDOWS = 8

RO_OK = 0
_ERR_NAMES = {-1: "RO_ERR_INVALID", -2: "RO_ERR_UNSUPPORTED", -3: "RO_ERR_HIP", -4: "RO_ERR_NOMEM",
              -5: "RO_ERR_STATE"}


class StftError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s (%d): %s" % (_ERR_NAMES.get(code, "RO_ERR"), code, text))
        self.code = code


class Bands(C.Structure):
    """ro_bands_t -- BolidRecorder::start's bin ranges (src/BolidRecorder.cpp:84-102)."""
    _fields_ = [("low_noise", C.c_int32), ("noise_width", C.c_int32), ("low_detect", C.c_int32),
                ("detect_width", C.c_int32), ("avg_bins", C.c_int32)]


class BandWindow(C.Structure):
    """ro_band_window_t -- one run of columns [first_col, first_col + cols) of the fft-shifted row."""
    _fields_ = [("first_col", C.c_int32), ("cols", C.c_int32)]

    def __iter__(self):                                 # first_col, cols = window
        return iter((self.first_col, self.cols))

    def __repr__(self):
        return "BandWindow(%d, %d)" % (self.first_col, self.cols)


class ScanRecord(C.Structure):
    """ro_scan_record_t -- (n, p, a) of BolidRecorder::update (src/BolidRecorder.cpp:121-132)."""
    _fields_ = [("noise", C.c_float), ("peak", C.c_int32), ("average", C.c_float)]


class Timing(C.Structure):
    """ro_stft_timing_t"""
    _fields_ = [("push_calls", C.c_int64), ("push_ms_avg", C.c_double), ("push_ms_max", C.c_double),
                ("batches", C.c_int64), ("batch_gpu_ms_avg", C.c_double), ("batch_gpu_ms_max", C.c_double),
                ("batch_rows", C.c_int64), ("row_gpu_us_avg", C.c_double),
                ("fetch_calls", C.c_int64), ("fetch_ms_avg", C.c_double), ("fetch_ms_max", C.c_double)]


SCAN_DTYPE = np.dtype([("noise", np.float32), ("peak", np.int32), ("average", np.float32)])


class Detector(C.Structure):
    """ro_detector_t -- advance_ and jitter_ of a BolidRecorder, in rows (src/BolidRecorder.cpp:100-101)."""
    _fields_ = [("advance", C.c_int32), ("jitter", C.c_int32)]


# ro_event_t (40 bytes), ro_detect_state_t (32, all zero = STATE_INIT), ro_detect_summary_t (24)
EVENT_DTYPE = np.dtype([("fire_row", np.int64), ("start_row", np.int64), ("length", np.int64), ("noise", np.float32),
                        ("peak", np.int32), ("magnitude", np.float32), ("reserved", np.int32)])
DETECT_STATE_DTYPE = np.dtype([("first_detect_row", np.int64), ("last_detect_row", np.int64), ("noise", np.float32),
                               ("peak", np.int32), ("magnitude", np.float32), ("open", np.int32)])
DETECT_SUMMARY_DTYPE = np.dtype([("events", np.int64), ("detect_rows", np.int64), ("marginal_rows", np.int64)])

RO_SNAP_CAPTURED, RO_SNAP_EMPTY, RO_SNAP_LOST = 0, 1, 2


class RowRing(C.Structure):
    """ro_row_ring_t (32 bytes) -- a ring of rows the caller owns: stream row r lives in slot r % ring_rows, `cols` floats
    of every `stride` (src/WaterfallBackend.cpp:107-127 reserves rows of such a ring for a snapshot)."""
    _fields_ = [("d_rows", C.c_void_p), ("stride", C.c_int64), ("ring_rows", C.c_int64), ("cols", C.c_int32),
                ("reserved", C.c_int32)]


ROW_RING = RowRing
# ro_snapshot_t (72 bytes: one resolved event) and ro_snap_summary_t (64, one per call)
SNAPSHOT_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_row", np.int64), ("offset", np.int64), ("rows", np.int32),
                           ("slot", np.int32), ("status", np.int32), ("reserved", np.int32)])
SNAP_SUMMARY_DTYPE = np.dtype([("resolved", np.int64), ("captured", np.int64), ("empty", np.int64), ("lost", np.int64),
                               ("pending", np.int64), ("pending_dropped", np.int64), ("unlisted", np.int64),
                               ("arena_floats", np.int64)])


RO_MAX_IQ_SPANS = 4


class IqSpan(C.Structure):
    """ro_iq_span_t (32 bytes) -- stream samples [first_sample, first_sample + samples) lie at d_iq, in `format`"""
    _fields_ = [("d_iq", C.c_void_p), ("first_sample", C.c_int64), ("samples", C.c_int64), ("format", C.c_int32),
                ("reserved", C.c_int32)]


# ro_raw_capture_t (72 bytes: one resolved candidate of the raw capture) and ro_raw_summary_t (64, one per call)
RAW_CAPTURE_DTYPE = np.dtype([("event", EVENT_DTYPE), ("first_sample", np.int64), ("samples", np.int64), ("offset", np.int64),
                              ("slot", np.int32), ("status", np.int32)])
RAW_SUMMARY_DTYPE = np.dtype([("resolved", np.int64), ("captured", np.int64), ("empty", np.int64), ("lost", np.int64),
                              ("pending", np.int64), ("pending_dropped", np.int64), ("arena_floats", np.int64),
                              ("reserved", np.int64)])

RO_FITS_BLOCK = 2880
RO_UNIT_WRITTEN, RO_UNIT_SKIPPED, RO_UNIT_NO_ROOM, RO_UNIT_INVALID = 0, 1, 2, 3
# ro_fits_unit_t (32 bytes: the data unit of source directory entry d) and ro_unit_summary_t (64, one per call)
FITS_UNIT_DTYPE = np.dtype([("offset", np.int64), ("bytes", np.int64), ("naxis2", np.int64), ("naxis1", np.int32),
                            ("status", np.int32)])
UNIT_SUMMARY_DTYPE = np.dtype([("entries", np.int64), ("written", np.int64), ("skipped", np.int64), ("no_room", np.int64),
                               ("invalid", np.int64), ("units_bytes", np.int64), ("needed_bytes", np.int64),
                               ("reserved", np.int64)])

RO_MAX_PERIODIC = 8
RO_PERIODIC_WRITTEN, RO_PERIODIC_LOST, RO_PERIODIC_NO_ROOM = 0, 1, 2
# ro_periodic_t (12 bytes: one periodic recorder), ro_periodic_entry_t (56: one snapshot of one recorder) and
# ro_periodic_summary_t (64, one per plan)
PERIODIC_DTYPE = np.dtype([("snapshot_rows", np.int32), ("first_col", np.int32), ("cols", np.int32)])
PERIODIC_ENTRY_DTYPE = np.dtype([("index", np.int64), ("first_row", np.int64), ("due_row", np.int64), ("offset", np.int64),
                                 ("bytes", np.int64), ("rows", np.int32), ("naxis1", np.int32), ("recorder", np.int32),
                                 ("status", np.int32)])
PERIODIC_SUMMARY_DTYPE = np.dtype([("entries", np.int64), ("written", np.int64), ("lost", np.int64), ("no_room", np.int64),
                                   ("unlisted", np.int64), ("units_bytes", np.int64), ("needed_bytes", np.int64),
                                   ("reserved", np.int64)])

RO_LEVEL_BLOCK = 720
# ro_level_range_t (8 bytes: the colour range of one level image)
LEVEL_RANGE_DTYPE = np.dtype([("ln_min", np.float32), ("ln_max", np.float32)])
# ro_resize_info_t (64 bytes: the host scalars of one resize plan)
RESIZE_INFO_DTYPE = np.dtype([("jobs", np.int64), ("h_items", np.int64), ("v_items", np.int64), ("mid_bytes", np.int64),
                              ("plan_bytes", np.int64), ("reserved", np.int64, (3,))])


class Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("bins", C.c_int32), ("overlap", C.c_int32),
                ("sample_rate", C.c_int32), ("window_kind", C.c_int32),
                ("window_table", C.POINTER(C.c_float)), ("iq_gain", C.c_double),
                ("iq_phase_shift", C.c_int32), ("device", C.c_int32), ("max_batch_rows", C.c_int32),
                ("enable_scan", C.c_int32), ("bands", Bands), ("tile_first_col", C.c_int32),
                ("tile_cols", C.c_int32), ("spare_cus_per_xcd", C.c_int32), ("precision", C.c_int32),
                ("tile_ln", C.c_int32)]


_EXPORTS = {
    # name: (restype, argtypes)
    "ro_abi_version": (C.c_int, []),
    "ro_last_error": (C.c_char_p, []),
    "ro_device_count": (C.c_int, []),
    "ro_clamp_overlap": (C.c_int, [C.c_int, C.c_int]),
    "ro_fft_sample_rate": (C.c_float, [C.c_int, C.c_int, C.c_int]),
    "ro_frequency_to_bin": (C.c_int, [C.c_int, C.c_int, C.c_float]),
    "ro_bin_to_frequency": (C.c_float, [C.c_int, C.c_int, C.c_int]),
    "ro_time_to_fft_samples": (C.c_int, [C.c_double, C.c_float]),
    "ro_row_count": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "ro_window_table": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "ro_bins_supported": (C.c_int, [C.c_int]),
    "ro_shard_rows": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ro_shard_samples": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]),
    "ro_shard_max_rows": (C.c_int64, [C.c_int64, C.c_int]),
    "ro_stitch_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_void_p]),
    "ro_direct_schedule": (C.c_int, [C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ro_allgather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_gather_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                 C.c_void_p, C.c_void_p]),
    "ro_allgather_rows_direct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_size_t,
                                           C.c_void_p, C.c_void_p]),
    "ro_stitch_rows_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "ro_stft_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "ro_stft_destroy": (C.c_int, [C.c_void_p]),
    "ro_stft_get_window": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "ro_stft_hop": (C.c_int, [C.c_void_p]),
    "ro_stft_bins": (C.c_int, [C.c_void_p]),
    "ro_stft_device_name": (C.c_int, [C.c_void_p, C.c_char_p, C.c_size_t]),
    "ro_stft_set_bands": (C.c_int, [C.c_void_p, C.POINTER(Bands)]),
    "ro_stft_set_extra_bands": (C.c_int, [C.c_void_p, C.POINTER(Bands), C.c_int]),
    "ro_stft_extra_bands": (C.c_int, [C.c_void_p, C.POINTER(Bands)]),
    "ro_stft_run_resident_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_scan_sets_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "ro_stft_fetch_sets": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float),
                                     C.POINTER(ScanRecord), C.POINTER(ScanRecord), C.POINTER(C.c_int64),
                                     C.POINTER(C.c_int64)]),
    "ro_stft_run_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_run_resident_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "ro_ln_levels": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p]),
    "ro_stft_fetch_ln": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ro_stft_spectra_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_scan_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                        C.c_void_p]),
    "ro_stft_ln_tile_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_band_supported": (C.c_int, [C.c_int, C.c_int]),
    "ro_stft_band_supported_precision": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "ro_bands_hull": (C.c_int, [C.POINTER(Bands), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ro_stft_band_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                                        C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_stft_band_windows_supported": (C.c_int, [C.c_int, C.POINTER(BandWindow), C.c_int, C.c_int]),
    "ro_bands_windows": (C.c_int, [C.POINTER(Bands), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(BandWindow),
                                   C.POINTER(C.c_int)]),
    "ro_stft_band_windows_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                                C.POINTER(BandWindow), C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "ro_tile_windows_supported": (C.c_int, [C.c_int, C.POINTER(BandWindow), C.c_int]),
    "ro_merge_windows": (C.c_int, [C.POINTER(BandWindow), C.c_int, C.c_int, C.POINTER(BandWindow), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int32)]),
    "ro_stft_cut_windows_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(BandWindow),
                                               C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_run_resident_windows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                               C.c_void_p, C.c_int64, C.POINTER(BandWindow), C.c_int, C.c_void_p,
                                               C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_set_tile_windows": (C.c_int, [C.c_void_p, C.POINTER(BandWindow), C.c_int]),
    "ro_stft_tile_windows": (C.c_int, [C.c_void_p, C.POINTER(BandWindow)]),
    "ro_events_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(Detector), C.c_void_p, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_stft_events_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(Detector),
                                          C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_run_resident_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p,
                                              C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Detector),
                                              C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "ro_stft_ring_put_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(RowRing),
                                            C.c_void_p]),
    "ro_stft_snapshots_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32),
                                             C.POINTER(RowRing), C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_snapshots_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(RowRing),
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "ro_stft_raw_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(IqSpan), C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_raw_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(IqSpan), C.c_int,
                              C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_snapshot_units_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                                  C.POINTER(BandWindow), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                  C.c_void_p]),
    "ro_stft_raw_units_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_snapshot_units_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                         C.POINTER(BandWindow), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_raw_units_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p]),
    "ro_snapshot_rows": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ro_periodic_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int32, C.c_int64,
                                   C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_periodic_units_resident": (C.c_int, [C.c_void_p, C.POINTER(RowRing), C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_periodic_units_host": (C.c_int, [C.POINTER(RowRing), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "ro_stft_snapshot_levels_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                                   C.POINTER(BandWindow), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_void_p]),
    "ro_snapshot_levels_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                          C.POINTER(BandWindow), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_periodic_levels_resident": (C.c_int, [C.c_void_p, C.POINTER(RowRing), C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_periodic_levels_host": (C.c_int, [C.POINTER(RowRing), C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_int64]),
    "ro_png_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "ro_stft_levels_png_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_levels_png_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "ro_stft_levels_png_deflate_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                                      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_levels_png_deflate_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                             C.c_int64, C.c_void_p]),
    "ro_periodic_level_dir": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ro_resize_shape": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "ro_resize_plan": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_int64, C.c_void_p]),
    "ro_stft_levels_resize_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                 C.c_void_p]),
    "ro_levels_resize_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    "ro_stft_time_resident": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ro_stft_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.POINTER(C.c_int64)]),
    "ro_stft_flush": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ro_stft_fetch": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_float),
                                C.POINTER(ScanRecord), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ro_stft_reset": (C.c_int, [C.c_void_p]),
    "ro_stft_rows_complete": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ro_stft_set_row_sink": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    "ro_pinned_alloc": (C.c_void_p, [C.c_int, C.c_size_t]),
    "ro_pinned_free": (None, [C.c_void_p]),
    "ro_pinned_check": (C.c_int, [C.c_void_p, C.c_size_t]),
    "ro_stft_timing": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "ro_stft_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
}

_lib = None


def library_path():
    return _build.LIB


def exported_symbols():
    return sorted(_EXPORTS)


def hip_runtimes():
    """Paths of every libamdhip64 mapped into this process.  libro_stft.so asks the loader for `libamdhip64.so.7`; a
    copy some other package has already loaded under that SONAME (torch bundles one) is reused, so a process that
    imports torch FIRST holds one runtime.  The other order leaves two -- torch asks for its own copy by file name --
    and then a device pointer, a stream or page-locked memory of one runtime means nothing to the other."""
    found = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if "libamdhip64" in os.path.basename(path):
                    found.add(os.path.realpath(path))
    except OSError:
        pass
    return sorted(found)


def require_one_hip_runtime():
    """Raise when two HIP runtimes share the process (see hip_runtimes): handles are refused rather than handed
    pointers the other runtime owns."""
    rts = hip_runtimes()
    if len(rts) > 1:
        raise StftError(-5, "two HIP runtimes are mapped into this process (%s): import torch BEFORE radio-observer_amd "
                            "loads libro_stft.so, so that both use the same one" % ", ".join(rts))


def library():
    """Load libro_stft.so (building it first if the sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("RO_STFT_LIB")           # diagnostic builds (tools/ablate.sh) only
    if not path:
        path = _build.LIB
        if not os.path.exists(path):
            _build.build()
    lib = C.CDLL(path)
    for name, (res, args) in _EXPORTS.items():
        fn = getattr(lib, name)       # AttributeError here = symbol missing from the .so
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PinnedArray:
    """a float32 numpy view [rows, cols] of page-locked host memory from ro_pinned_alloc (freed with the object)"""

    def __init__(self, rows, cols, device=0):
        n = rows * cols * 4
        self._p = library().ro_pinned_alloc(device, n)
        if not self._p:
            raise MemoryError("ro_pinned_alloc(%d bytes) failed" % n)
        self.array = np.ctypeslib.as_array((C.c_float * (rows * cols)).from_address(self._p)).reshape(rows, cols)

    def close(self):
        if self._p:
            self.array = None
            library().ro_pinned_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check(rc):
    if rc != RO_OK:
        raise StftError(rc, (library().ro_last_error() or b"").decode("utf-8", "replace"))


# ---- host helpers -------------------------------------------------------------
def clamp_overlap(bins, overlap):
    return library().ro_clamp_overlap(bins, overlap)


def fft_sample_rate(sample_rate, bins, overlap):
    return library().ro_fft_sample_rate(sample_rate, bins, overlap)


def frequency_to_bin(bins, sample_rate, frequency):
    return library().ro_frequency_to_bin(bins, sample_rate, frequency)


def bin_to_frequency(bins, sample_rate, bin_):
    return library().ro_bin_to_frequency(bins, sample_rate, bin_)


def time_to_fft_samples(seconds, fft_rate):
    return library().ro_time_to_fft_samples(seconds, fft_rate)


def row_count(samples, bins, overlap):
    return int(library().ro_row_count(int(samples), bins, overlap))


def window_table(kind, bins):
    w = np.empty(bins, dtype=np.float32)
    _check(library().ro_window_table(kind, bins, w.ctypes.data_as(C.POINTER(C.c_float))))
    return w


def shard_rows(total_rows, world, rank):
    """(first_row, rows) of `rank` -- ro_shard_rows"""
    first, rows = C.c_int64(), C.c_int64()
    _check(library().ro_shard_rows(int(total_rows), world, rank, C.byref(first), C.byref(rows)))
    return first.value, rows.value


def shard_samples(first_row, rows, bins, overlap):
    """(first_sample, samples) a shard must hold, halo included -- ro_shard_samples"""
    s0, ns = C.c_int64(), C.c_int64()
    _check(library().ro_shard_samples(int(first_row), int(rows), bins, overlap, C.byref(s0), C.byref(ns)))
    return s0.value, ns.value


def shard_max_rows(total_rows, world):
    n = library().ro_shard_max_rows(int(total_rows), world)
    if n < 0:
        _check(int(n))
    return int(n)


def direct_schedule(world, rank, total_rows, k):
    """(to, from, recv_first_row, recv_rows) of step k of the direct exchange -- ro_direct_schedule"""
    to, frm = C.c_int(), C.c_int()
    f, n = C.c_int64(), C.c_int64()
    _check(library().ro_direct_schedule(world, rank, int(total_rows), k, C.byref(to), C.byref(frm), C.byref(f), C.byref(n)))
    return to.value, frm.value, f.value, n.value


def stitch_rows(gathered, total_rows, world):
    """numpy [world * max_rows, ...] (equal-block all-gather result) -> [total_rows, ...] in row order"""
    g = np.ascontiguousarray(gathered)
    row_bytes = g.strides[0]
    out = np.empty((int(total_rows),) + g.shape[1:], dtype=g.dtype)
    _check(library().ro_stitch_rows(C.c_void_p(g.ctypes.data), int(total_rows), world, row_bytes,
                                    C.c_void_p(out.ctypes.data)))
    return out


def ln_levels(ln, mn, mx):
    """the viewer's grey levels of log values given the image's range -- ro_ln_levels (host)"""
    a = np.ascontiguousarray(ln, dtype=np.float32)
    out = np.empty(a.shape, np.uint8)
    _check(library().ro_ln_levels(C.c_void_p(a.ctypes.data), a.size, float(mn), float(mx), C.c_void_p(out.ctypes.data)))
    return out


def bins_supported(bins):
    return bool(library().ro_bins_supported(bins))


def band_supported(bins, cols, precision=RO_PRECISION_F32):
    """whether Stft.band_resident can produce `cols` columns of a `bins`-bin row on a handle of `precision` --
    ro_stft_band_supported_precision (RO_PRECISION_F64: 131072 bins and above)"""
    return bool(library().ro_stft_band_supported_precision(bins, cols, precision))


def bands_hull(bands, bins, tile_first_col=0, tile_cols=0):
    """(first_col, cols) of the smallest column range that holds everything the recorders read -- ro_bands_hull"""
    first, cols = C.c_int(), C.c_int()
    _check(library().ro_bands_hull(C.byref(bands), bins, tile_first_col, tile_cols, C.byref(first), C.byref(cols)))
    return first.value, cols.value


def _windows(windows):
    """a ctypes array of BandWindow from BandWindow objects or (first_col, cols) pairs"""
    items = [w if isinstance(w, BandWindow) else BandWindow(*w) for w in windows]
    return (BandWindow * max(len(items), 1))(*items), len(items)


def band_windows_supported(bins, windows, precision=RO_PRECISION_F32):
    """whether Stft.band_windows_resident can produce these windows (BandWindow or (first_col, cols) each) of a
    `bins`-bin row on a handle of `precision` -- ro_stft_band_windows_supported"""
    arr, n = _windows(windows)
    return bool(library().ro_stft_band_windows_supported(bins, arr, n, precision))


def bands_windows(sets, bins, tile_first_col=0, tile_cols=0):
    """the windows (a list of BandWindow, ascending) that hold what the band sets `sets` (one Bands or a sequence of 1 ... 8)
    and the tile read of a row, kept apart where they lie apart -- ro_bands_windows"""
    sets = [sets] if isinstance(sets, Bands) else list(sets)
    arr = (Bands * max(len(sets), 1))(*sets)
    out, n = (BandWindow * RO_MAX_BAND_WINDOWS)(), C.c_int()
    _check(library().ro_bands_windows(arr, len(sets), bins, tile_first_col, tile_cols, out, C.byref(n)))
    return [BandWindow(out[i].first_col, out[i].cols) for i in range(n.value)]


def tile_windows_supported(bins, windows):
    """whether these windows (BandWindow or (first_col, cols) each) can be cut from a `bins`-bin full row: 1 ... 8 of
    them, ascending, not overlapping, inside the row -- ro_tile_windows_supported"""
    arr, n = _windows(windows)
    return bool(library().ro_tile_windows_supported(bins, arr, n))


def merge_windows(ranges, bins):
    """(windows, offsets): the tile windows (a list of BandWindow, ascending, at most 8) that hold the recorders' column
    ranges `ranges` (1 ... 32 of BandWindow or (first_col, cols), any order, overlaps allowed), and for each range the
    image column where its first column sits -- ro_merge_windows"""
    arr, n = _windows(ranges)
    out, count = (BandWindow * RO_MAX_TILE_WINDOWS)(), C.c_int()
    offs = (C.c_int32 * max(n, 1))()
    _check(library().ro_merge_windows(arr, n, bins, out, C.byref(count), offs))
    return [BandWindow(out[i].first_col, out[i].cols) for i in range(count.value)], [int(offs[i]) for i in range(n)]


def _detectors(detectors):
    """Detector or (advance, jitter) each -> ctypes array"""
    arr = (Detector * max(len(detectors), 1))()
    for i, d in enumerate(detectors):
        arr[i] = d if isinstance(d, Detector) else Detector(*d)
    return arr


def events_host(records, detector, first_row=0, state=None, capacity=None, want_detect=False):
    """BolidRecorder::update's decision and state machine over one set's records (a 1-D SCAN_DTYPE array, any stride: a
    column of a [row][set] array will do) -- ro_events_host.  detector: Detector or (advance, jitter).  state: a
    DETECT_STATE_DTYPE array of one entry, updated in place (None: a fresh one).  capacity: events kept (None: all).
    Returns (events, state, summary, detect): EVENT_DTYPE array of the events written, the state, a DETECT_SUMMARY_DTYPE
    scalar and the per-row decisions (uint8, or None)."""
    records = np.asarray(records)
    if records.dtype != SCAN_DTYPE or records.ndim != 1:
        raise ValueError("records: a one-dimensional SCAN_DTYPE array")
    rows = records.shape[0]
    stride = records.strides[0] // SCAN_DTYPE.itemsize if rows else 1
    if rows and (records.strides[0] % SCAN_DTYPE.itemsize or stride < 1):
        raise ValueError("records: a stride of whole records, ascending")
    if state is None:
        state = np.zeros(1, DETECT_STATE_DTYPE)
    cap = rows if capacity is None else capacity
    events = np.zeros(max(cap, 0), EVENT_DTYPE)
    summary = np.zeros(1, DETECT_SUMMARY_DTYPE)
    detect = np.zeros(rows, np.uint8) if want_detect else None
    det = _detectors([detector])
    _check(library().ro_events_host(C.c_void_p(records.ctypes.data) if rows else None, stride, first_row, rows, det,
                                    C.c_void_p(state.ctypes.data), C.c_void_p(events.ctypes.data) if cap > 0 else None,
                                    cap, C.c_void_p(summary.ctypes.data),
                                    C.c_void_p(detect.ctypes.data) if detect is not None and rows else None))
    return events[:min(int(summary["events"][0]), max(cap, 0))], state, summary[0], detect


def _snapshot_rows(snapshot_rows, slot_mask):
    """one int per slot up to the mask's highest bit (or one int for all of them) -> (ctypes int32 array, slots)"""
    slots = int(slot_mask).bit_length()
    if np.isscalar(snapshot_rows):
        snapshot_rows = [snapshot_rows] * slots
    if len(snapshot_rows) < slots:
        raise ValueError("snapshot_rows: one entry per slot up to the mask's highest bit, %d" % slots)
    return (C.c_int32 * max(slots, 1))(*[int(x) for x in snapshot_rows[:slots]]), slots


def snapshots_host(events, summary, slot_mask, snapshot_rows, ring, head_row, pending, pending_count, arena_floats,
                   cols=None):
    """The snapshots of one call over host memory -- ro_snapshots_host.  events: EVENT_DTYPE [slots, capacity] and summary:
    DETECT_SUMMARY_DTYPE [slots] as the events call leaves them (None, None: no events); ring: float32 [ring_rows, stride],
    stream row r in ring[r % ring_rows], `cols` floats of it (None: stride); pending: EVENT_DTYPE [slots, pending_capacity]
    and pending_count: int64 [slots], both updated in place.  Returns (directory, arena, summary): the SNAPSHOT_DTYPE
    entries resolved, the arena floats used, a SNAP_SUMMARY_DTYPE scalar."""
    rows_arr, slots = _snapshot_rows(snapshot_rows, slot_mask)
    ring = np.asarray(ring)
    if ring.dtype != np.float32 or ring.ndim != 2 or not ring.flags.c_contiguous:
        raise ValueError("ring: a C-contiguous float32 array [ring_rows, stride]")
    desc = RowRing(ring.ctypes.data, ring.shape[1], ring.shape[0], ring.shape[1] if cols is None else cols, 0)
    capacity = 0 if events is None else events.shape[1]
    if events is not None and (events.dtype != EVENT_DTYPE or events.ndim != 2 or events.shape[0] < slots or
                               not events.flags.c_contiguous or summary is None or summary.dtype != DETECT_SUMMARY_DTYPE or
                               summary.shape[0] < slots):
        raise ValueError("events: EVENT_DTYPE [slots, capacity] with summary: DETECT_SUMMARY_DTYPE [slots]")
    if (pending.dtype != EVENT_DTYPE or pending.ndim != 2 or pending.shape[0] < slots or not pending.flags.c_contiguous or
            pending_count.dtype != np.int64 or pending_count.shape[0] < slots):
        raise ValueError("pending: EVENT_DTYPE [slots, pending_capacity] with pending_count: int64 [slots]")
    pcap = pending.shape[1]
    directory = np.zeros(max(slots * (capacity + pcap), 1), SNAPSHOT_DTYPE)
    arena = np.zeros(max(arena_floats, 1), np.float32)
    out = np.zeros(1, SNAP_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_snapshots_host(p(events) if capacity else None, capacity, p(summary) if summary is not None else None,
                                       slot_mask, rows_arr, C.byref(desc), head_row, p(pending) if pcap else None,
                                       p(pending_count), pcap, p(directory), p(arena) if arena_floats > 0 else None,
                                       arena_floats, p(out)))
    return directory[:int(out["resolved"][0])], arena[:int(out["arena_floats"][0])], out[0]


def _spans(spans):
    """IqSpan or (address, first_sample, samples, format) each -> (ctypes array, count)"""
    spans = list(spans)
    arr = (IqSpan * max(len(spans), 1))()
    for i, sp in enumerate(spans):
        arr[i] = sp if isinstance(sp, IqSpan) else IqSpan(None if sp[0] is None else _ptr(sp[0]).value, sp[1], sp[2], sp[3], 0)
    return arr, len(spans)


def raw_host(bins, overlap, sample_rate, directory, snap_summary, spans, pending, pending_count, arena_floats):
    """The raw I/Q runs of one call over host memory -- ro_raw_host.  directory: SNAPSHOT_DTYPE entries and snap_summary: a
    SNAP_SUMMARY_DTYPE array of one entry, as the snapshots call leaves them; spans: [(array, first_sample, format), ...] of
    numpy arrays that hold whole samples (float32 / int16 / float64, two numbers each); pending: SNAPSHOT_DTYPE
    [pending_capacity] and pending_count: int64 [1], both updated in place.  Returns (raw directory, arena, summary): the
    RAW_CAPTURE_DTYPE entries resolved, the arena floats used, a RAW_SUMMARY_DTYPE scalar."""
    directory = np.ascontiguousarray(directory)
    if directory.dtype != SNAPSHOT_DTYPE or directory.ndim != 1 or snap_summary.dtype != SNAP_SUMMARY_DTYPE:
        raise ValueError("directory: SNAPSHOT_DTYPE [n] with snap_summary: SNAP_SUMMARY_DTYPE [1]")
    if (pending.dtype != SNAPSHOT_DTYPE or pending.ndim != 1 or not pending.flags.c_contiguous or
            pending_count.dtype != np.int64 or pending_count.size < 1):
        raise ValueError("pending: SNAPSHOT_DTYPE [pending_capacity] with pending_count: int64 [1]")
    item = {RO_IQ_F32: 8, RO_IQ_I16: 4, RO_IQ_F64: 16}
    keep, desc = [], []
    for array, first_sample, fmt in spans:
        array = np.ascontiguousarray(array)
        keep.append(array)
        desc.append(IqSpan(array.ctypes.data, first_sample, array.nbytes // item.get(fmt, 8), fmt, 0))
    arr, count = _spans(desc)
    dcap, pcap = directory.shape[0], pending.shape[0]
    raw_dir = np.zeros(max(dcap + pcap, 1), RAW_CAPTURE_DTYPE)
    arena = np.zeros(max(arena_floats, 1), np.float32)
    out = np.zeros(1, RAW_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_raw_host(bins, overlap, sample_rate, p(directory) if dcap else None, dcap, p(snap_summary), arr, count,
                                 p(pending) if pcap else None, p(pending_count), pcap, p(raw_dir),
                                 p(arena) if arena_floats > 0 else None, arena_floats, p(out)))
    return raw_dir[:int(out["resolved"][0])], arena[:int(out["arena_floats"][0])], out[0]


def _slot_windows(slot_windows):
    """BandWindow or (first_col, cols) per slot, None for a slot whose files are not wanted -> a ctypes array of
    1 + RO_MAX_EXTRA_BANDS windows (the slots that are not named: not wanted)"""
    slot_windows = list(slot_windows)
    if len(slot_windows) > 1 + RO_MAX_EXTRA_BANDS:
        raise ValueError("slot_windows: at most one per slot, %d" % (1 + RO_MAX_EXTRA_BANDS))
    arr = (BandWindow * (1 + RO_MAX_EXTRA_BANDS))()
    for i, w in enumerate(slot_windows):
        if w is not None:
            arr[i] = w if isinstance(w, BandWindow) else BandWindow(int(w[0]), int(w[1]))
    return arr


def _units_host(call, directory, dtype, summary, arena, units_bytes, *middle):
    directory = np.ascontiguousarray(directory)
    if directory.dtype != dtype or directory.ndim != 1 or summary.itemsize != 64 or summary.size < 1:
        raise ValueError("directory: %d-byte entries [n] with the summary of the call that wrote them" % dtype.itemsize)
    arena = np.ascontiguousarray(arena)
    if arena.dtype != np.float32 or arena.ndim != 1:
        raise ValueError("arena: float32 [arena_floats]")
    dcap = directory.shape[0]
    unit_dir = np.zeros(max(dcap, 1), FITS_UNIT_DTYPE)
    units = np.zeros(max(units_bytes, 1), np.uint8)
    out = np.zeros(1, UNIT_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(call(p(directory) if dcap else None, dcap, p(summary), p(arena) if arena.size else None, arena.size, *middle,
                p(unit_dir), p(units) if units_bytes > 0 else None, units_bytes, p(out)))
    return unit_dir[:int(out["entries"][0])], units[:int(out["units_bytes"][0])], out[0]


def snapshot_units_host(directory, snap_summary, arena, cols, slot_windows, units_bytes):
    """The FITS data units of one snapshot arena over host memory -- ro_snapshot_units_host.  directory: SNAPSHOT_DTYPE
    entries and snap_summary: a SNAP_SUMMARY_DTYPE array of one entry, as the snapshots call leaves them; arena: float32,
    rows of `cols` floats; slot_windows: (first_col, cols) of each slot's recorder in the image, None: not wanted.
    Returns (unit directory, units, summary): one FITS_UNIT_DTYPE entry per directory entry, the bytes of the units in
    use, a UNIT_SUMMARY_DTYPE scalar."""
    return _units_host(library().ro_snapshot_units_host, directory, SNAPSHOT_DTYPE, snap_summary, arena, units_bytes, cols,
                       _slot_windows(slot_windows))


def raw_units_host(raw_directory, raw_summary, arena, units_bytes):
    """The FITS data units of one raw arena over host memory -- ro_raw_units_host.  raw_directory: RAW_CAPTURE_DTYPE entries
    and raw_summary: a RAW_SUMMARY_DTYPE array of one entry, as the raw call leaves them.  Returns as snapshot_units_host."""
    return _units_host(library().ro_raw_units_host, raw_directory, RAW_CAPTURE_DTYPE, raw_summary, arena, units_bytes)


def snapshot_rows(sample_rate, bins, overlap, snapshot_length):
    """snapshotRows_ of a periodic recorder -- ro_snapshot_rows (src/WaterfallBackend.cpp:339-345)"""
    return library().ro_snapshot_rows(sample_rate, bins, overlap, snapshot_length)


def periodic_recorders(recorders):
    """a PERIODIC_DTYPE array, or (snapshot_rows, first_col, cols) per recorder -> a C-contiguous PERIODIC_DTYPE array"""
    if isinstance(recorders, np.ndarray) and recorders.dtype == PERIODIC_DTYPE:
        return np.ascontiguousarray(recorders)
    out = np.zeros(len(recorders), PERIODIC_DTYPE)
    for i, r in enumerate(recorders):
        out[i] = tuple(int(x) for x in r)
    return out


def periodic_plan(recorders, next_index, head_row, final, ring_rows, cols, units_bytes, capacity):
    """What the periodic recorders have to write at head_row -- ro_periodic_plan, pure host arithmetic.  recorders: see
    periodic_recorders; next_index: int64 [count], zero-filled once, updated in place.  Returns (directory, summary): the
    PERIODIC_ENTRY_DTYPE entries listed and a PERIODIC_SUMMARY_DTYPE scalar."""
    recs = periodic_recorders(recorders)
    if not isinstance(next_index, np.ndarray) or next_index.dtype != np.int64 or next_index.ndim != 1 or \
            next_index.shape[0] < len(recs) or not next_index.flags.c_contiguous:
        raise ValueError("next_index: a C-contiguous int64 array [count]")
    directory = np.zeros(max(capacity, 1), PERIODIC_ENTRY_DTYPE)
    out = np.zeros(1, PERIODIC_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_periodic_plan(p(recs) if len(recs) else None, len(recs), p(next_index), head_row, 1 if final else 0,
                                      ring_rows, cols, units_bytes, p(directory) if capacity > 0 else None, capacity, p(out)))
    return directory[:int(out["entries"][0])], out[0]


def periodic_units_host(ring, recorders, directory, units_bytes, cols=None):
    """The FITS data units of one plan over host memory -- ro_periodic_units_host.  ring: float32 [ring_rows, stride], stream
    row r in ring[r % ring_rows], `cols` floats of it (None: stride); directory: PERIODIC_ENTRY_DTYPE entries as
    periodic_plan returned them.  Returns the bytes of the units in use."""
    ring = np.asarray(ring)
    if ring.dtype != np.float32 or ring.ndim != 2 or not ring.flags.c_contiguous:
        raise ValueError("ring: a C-contiguous float32 array [ring_rows, stride]")
    desc = RowRing(ring.ctypes.data, ring.shape[1], ring.shape[0], ring.shape[1] if cols is None else cols, 0)
    recs = periodic_recorders(recorders)
    directory = np.ascontiguousarray(directory)
    if directory.dtype != PERIODIC_ENTRY_DTYPE or directory.ndim != 1:
        raise ValueError("directory: PERIODIC_ENTRY_DTYPE [entries]")
    units = np.zeros(max(units_bytes, 1), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_periodic_units_host(C.byref(desc), p(recs) if len(recs) else None, len(recs),
                                            p(directory) if len(directory) else None, len(directory),
                                            p(units) if units_bytes > 0 else None, units_bytes))
    written = directory[directory["status"] == RO_PERIODIC_WRITTEN]
    used = 0 if not len(written) else int(written[-1]["offset"]) + -(-int(written[-1]["bytes"]) // RO_FITS_BLOCK) * RO_FITS_BLOCK
    return units[:used]


def snapshot_levels_host(directory, snap_summary, arena, cols, slot_windows, levels_bytes):
    """The grey-level previews of one snapshot arena over host memory -- ro_snapshot_levels_host.  The arguments of
    snapshot_units_host, the room in level bytes.  Returns (level directory, ranges, levels, summary): one FITS_UNIT_DTYPE
    entry (offsets and bytes in level terms) and one LEVEL_RANGE_DTYPE entry per directory entry, the bytes of the images
    in use (each naxis1 x naxis2 uint8, zero-padded to 720), a UNIT_SUMMARY_DTYPE scalar."""
    directory = np.ascontiguousarray(directory)
    if directory.dtype != SNAPSHOT_DTYPE or directory.ndim != 1 or snap_summary.itemsize != 64 or snap_summary.size < 1:
        raise ValueError("directory: SNAPSHOT_DTYPE [n] with the summary of the call that wrote them")
    arena = np.ascontiguousarray(arena)
    if arena.dtype != np.float32 or arena.ndim != 1:
        raise ValueError("arena: float32 [arena_floats]")
    dcap = directory.shape[0]
    level_dir = np.zeros(max(dcap, 1), FITS_UNIT_DTYPE)
    ranges = np.zeros(max(dcap, 1), LEVEL_RANGE_DTYPE)
    levels = np.zeros(max(levels_bytes, 1), np.uint8)
    out = np.zeros(1, UNIT_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_snapshot_levels_host(p(directory) if dcap else None, dcap, p(snap_summary), p(arena) if arena.size else None,
                                             arena.size, cols, _slot_windows(slot_windows), p(level_dir), p(ranges),
                                             p(levels) if levels_bytes > 0 else None, levels_bytes, p(out)))
    n = int(out["entries"][0])
    return level_dir[:n], ranges[:n], levels[:int(out["units_bytes"][0])], out[0]


def periodic_levels_host(ring, recorders, directory, levels_bytes, cols=None):
    """The grey-level previews of one periodic plan over host memory -- ro_periodic_levels_host.  The arguments of
    periodic_units_host, the room in level bytes (a quarter of the units').  Returns (ranges, levels): one LEVEL_RANGE_DTYPE
    entry per directory entry (zero where the entry is not WRITTEN) and the bytes of the images in use; the image of a
    WRITTEN entry e starts at e["offset"] // 4."""
    ring = np.asarray(ring)
    if ring.dtype != np.float32 or ring.ndim != 2 or not ring.flags.c_contiguous:
        raise ValueError("ring: a C-contiguous float32 array [ring_rows, stride]")
    desc = RowRing(ring.ctypes.data, ring.shape[1], ring.shape[0], ring.shape[1] if cols is None else cols, 0)
    recs = periodic_recorders(recorders)
    directory = np.ascontiguousarray(directory)
    if directory.dtype != PERIODIC_ENTRY_DTYPE or directory.ndim != 1:
        raise ValueError("directory: PERIODIC_ENTRY_DTYPE [entries]")
    ranges = np.zeros(max(len(directory), 1), LEVEL_RANGE_DTYPE)
    levels = np.zeros(max(levels_bytes, 1), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_periodic_levels_host(C.byref(desc), p(recs) if len(recs) else None, len(recs),
                                             p(directory) if len(directory) else None, len(directory), p(ranges),
                                             p(levels) if levels_bytes > 0 else None, levels_bytes))
    written = directory[directory["status"] == RO_PERIODIC_WRITTEN]
    used = 0 if not len(written) else (int(written[-1]["offset"]) + -(-int(written[-1]["bytes"]) // RO_FITS_BLOCK) * RO_FITS_BLOCK) // 4
    return ranges[:len(directory)], levels[:used]


RO_PNG_ALIGN = 16


def png_bytes(naxis1, naxis2):
    """The bytes of the PNG of a naxis1 x naxis2 level image in stored deflate blocks -- ro_png_bytes: 63 + 5 blocks + raw
    bytes.  Raises for a shape that cannot be a PNG."""
    n = int(library().ro_png_bytes(int(naxis1), int(naxis2)))
    if n < 0:
        _check(n)
    return n


def _levels_png_host(call, level_dir, level_summary, levels, png_room, dir_capacity):
    level_dir = np.ascontiguousarray(level_dir)
    level_summary = np.ascontiguousarray(level_summary).reshape(-1)
    if level_dir.dtype != FITS_UNIT_DTYPE or level_dir.ndim != 1 or level_summary.dtype != UNIT_SUMMARY_DTYPE or level_summary.size < 1:
        raise ValueError("level_dir: FITS_UNIT_DTYPE [n] with the UNIT_SUMMARY_DTYPE of the call that wrote them")
    levels = np.ascontiguousarray(levels)
    if levels.dtype != np.uint8 or levels.ndim != 1:
        raise ValueError("levels: uint8 [levels_bytes]")
    dcap = level_dir.shape[0] if dir_capacity is None else dir_capacity
    png_dir = np.zeros(max(dcap, 1), FITS_UNIT_DTYPE)
    png = np.zeros(max(png_room, 1), np.uint8)
    out = np.zeros(1, UNIT_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(call(p(level_dir) if dcap else None, dcap, p(level_summary), p(levels) if levels.size else None,
                levels.size, p(png_dir), p(png) if png_room > 0 else None, png_room, p(out)))
    return png_dir[:int(out["entries"][0])], png[:int(out["units_bytes"][0])], out[0]


def levels_png_host(level_dir, level_summary, levels, png_room, dir_capacity=None):
    """The preview files of one level directory over host memory -- ro_levels_png_host.  level_dir: FITS_UNIT_DTYPE entries in
    level terms and level_summary: the UNIT_SUMMARY_DTYPE of the call that wrote them (snapshot_levels_host, or
    periodic_level_dir); levels: uint8; png_room: the room in bytes; dir_capacity: entries of level_dir to look at (None: all).
    Returns (directory, files, summary): one FITS_UNIT_DTYPE entry per level entry (offset into the files, a multiple of 16;
    bytes: the file's exact size), the bytes of the files in use, a UNIT_SUMMARY_DTYPE scalar."""
    return _levels_png_host(library().ro_levels_png_host, level_dir, level_summary, levels, png_room, dir_capacity)


def levels_png_deflate_host(level_dir, level_summary, levels, png_room, dir_capacity=None):
    """The compressed preview files of one level directory over host memory -- ro_levels_png_deflate_host: the arguments and
    the return of levels_png_host, the files' deflate blocks Huffman coded where that is shorter, so a file's bytes depend on
    its levels and are at most png_bytes(naxis1, naxis2).  png_room = 0 is the sizing call: the summary's needed_bytes is the
    room that holds every writable file."""
    return _levels_png_host(library().ro_levels_png_deflate_host, level_dir, level_summary, levels, png_room, dir_capacity)


def periodic_level_dir(directory):
    """The directory periodic_plan returned, in the level form levels_png_host and Stft.levels_png_resident read --
    ro_periodic_level_dir.  Returns (level directory, summary): FITS_UNIT_DTYPE entries, a UNIT_SUMMARY_DTYPE scalar."""
    directory = np.ascontiguousarray(directory)
    if directory.dtype != PERIODIC_ENTRY_DTYPE or directory.ndim != 1:
        raise ValueError("directory: PERIODIC_ENTRY_DTYPE [entries]")
    level_dir = np.zeros(max(len(directory), 1), FITS_UNIT_DTYPE)
    out = np.zeros(1, UNIT_SUMMARY_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_periodic_level_dir(p(directory) if len(directory) else None, len(directory), p(level_dir), p(out)))
    return level_dir[:len(directory)], out[0]


def resize_shape(naxis1, naxis2, width):
    """The shape fits2png's --width gives a naxis1 x naxis2 image -- ro_resize_shape: (width, int(naxis2 * (width / naxis1)))
    where width < naxis1, the image's own shape otherwise.  The height can be 0."""
    w, h = C.c_int32(), C.c_int64()
    _check(library().ro_resize_shape(int(naxis1), int(naxis2), int(width), C.byref(w), C.byref(h)))
    return w.value, h.value


def resize_plan(level_dir, level_summary, levels_bytes, width, out_levels_bytes, dir_capacity=None):
    """The plan that resizes every level image of a HOST level directory to `width` -- ro_resize_plan, its sizing form first.
    level_dir / level_summary as levels_png_host takes them; levels_bytes: the room their offsets are checked against;
    out_levels_bytes: the room of the resized images.  Returns (out directory, out summary, plan, info): FITS_UNIT_DTYPE
    entries and a UNIT_SUMMARY_DTYPE scalar in the levels' form, for levels_png_host and Stft.levels_png_resident to read;
    the blob as uint8 [info.plan_bytes], to upload; a RESIZE_INFO_DTYPE array of one entry."""
    level_dir = np.ascontiguousarray(level_dir)
    level_summary = np.ascontiguousarray(level_summary).reshape(-1)
    if level_dir.dtype != FITS_UNIT_DTYPE or level_dir.ndim != 1 or level_summary.dtype != UNIT_SUMMARY_DTYPE or level_summary.size < 1:
        raise ValueError("level_dir: FITS_UNIT_DTYPE [n] with the UNIT_SUMMARY_DTYPE of the call that wrote them")
    dcap = level_dir.shape[0] if dir_capacity is None else dir_capacity
    out_dir = np.zeros(max(dcap, 1), FITS_UNIT_DTYPE)
    out = np.zeros(1, UNIT_SUMMARY_DTYPE)
    info = np.zeros(1, RESIZE_INFO_DTYPE)
    p = lambda a: C.c_void_p(a.ctypes.data)
    args = (p(level_dir) if dcap else None, dcap, p(level_summary), int(levels_bytes), int(width), p(out_dir), int(out_levels_bytes), p(out))
    _check(library().ro_resize_plan(*args, None, 0, p(info)))
    plan = np.zeros(int(info["plan_bytes"][0]) // 8, np.int64).view(np.uint8)
    _check(library().ro_resize_plan(*args, p(plan), plan.size, p(info)))
    return out_dir[:int(out["entries"][0])], out[0], plan, info


def levels_resize_host(info, plan, levels, out_levels_bytes):
    """The resized images of one plan over host memory -- ro_levels_resize_host.  info, plan: what resize_plan returned;
    levels: uint8, the images the planned directory describes.  Returns the out levels, uint8 [out_levels_bytes]: every
    written entry's image at its offset, zero-padded to its last 720-byte block."""
    info = np.ascontiguousarray(info).reshape(-1)
    plan, levels = np.ascontiguousarray(plan), np.ascontiguousarray(levels)
    if info.dtype != RESIZE_INFO_DTYPE or info.size < 1 or plan.dtype != np.uint8 or levels.dtype != np.uint8 or levels.ndim != 1:
        raise ValueError("info: RESIZE_INFO_DTYPE; plan, levels: uint8")
    out = np.zeros(max(out_levels_bytes, 1), np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    _check(library().ro_levels_resize_host(p(info), p(plan), p(levels) if levels.size else None, levels.size,
                                           p(out) if out_levels_bytes > 0 else None, out_levels_bytes))
    return out[:out_levels_bytes]


def device_count():
    n = library().ro_device_count()
    if n < 0:
        _check(n)
    return n


def _ptr(x):
    """int address, torch tensor (data_ptr) or None -> c_void_p."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


# ---- the handle ---------------------------------------------------------------
class Stft:
    """One STFT stream on one GPU (ro_stft_t)."""

    def __init__(self, bins=32768, overlap=0, sample_rate=48000, window=RO_WINDOW_NUTTALL,
                 window_table=None, iq_gain=0.0, iq_phase_shift=0, device=0, max_batch_rows=0,
                 bands=None, tile=None, spare_cus_per_xcd=0, precision=RO_PRECISION_F32, tile_ln=False,
                 extra_bands=None):
        cfg = Config()
        cfg.struct_size = C.sizeof(Config)
        cfg.bins, cfg.overlap, cfg.sample_rate = bins, overlap, sample_rate
        cfg.window_kind = window
        self._wt = None
        if window_table is not None:
            self._wt = np.ascontiguousarray(window_table, dtype=np.float32)
            if self._wt.size != bins:
                raise ValueError("window_table must have `bins` entries")
            cfg.window_kind = RO_WINDOW_CUSTOM
            cfg.window_table = self._wt.ctypes.data_as(C.POINTER(C.c_float))
        cfg.iq_gain = iq_gain
        cfg.iq_phase_shift = iq_phase_shift
        cfg.device = device
        cfg.max_batch_rows = max_batch_rows
        if bands is not None:
            cfg.enable_scan = 1
            cfg.bands = bands
        if tile is not None:
            cfg.tile_first_col, cfg.tile_cols = tile
        cfg.spare_cus_per_xcd = spare_cus_per_xcd
        cfg.precision = precision
        cfg.tile_ln = 1 if tile_ln else 0
        self._h = C.c_void_p()
        lib = library()
        require_one_hip_runtime()
        _check(lib.ro_stft_create(C.byref(cfg), C.byref(self._h)))
        self.bins = bins
        self.hop = library().ro_stft_hop(self._h)
        self.scan_enabled = bands is not None
        self.tile = tile
        self.extra_count = 0
        self.image_cols = 0                              # columns of the tile windows' image (0: no windows set)
        if extra_bands:
            try:
                self.set_extra_bands(extra_bands)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            library().ro_stft_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def window(self):
        w = np.empty(self.bins, dtype=np.float32)
        _check(library().ro_stft_get_window(self._h, w.ctypes.data_as(C.POINTER(C.c_float))))
        return w

    @property
    def device_name(self):
        buf = C.create_string_buffer(256)
        _check(library().ro_stft_device_name(self._h, buf, 256))
        return buf.value.decode()

    def set_bands(self, bands):
        _check(library().ro_stft_set_bands(self._h, C.byref(bands)))
        self.scan_enabled = True

    def set_extra_bands(self, sets):
        """up to RO_MAX_EXTRA_BANDS more band sets scanned for every row beside the primary (one per further detector);
        an empty list removes them -- ro_stft_set_extra_bands"""
        sets = list(sets or [])
        arr = (Bands * max(len(sets), 1))(*sets)
        _check(library().ro_stft_set_extra_bands(self._h, arr, len(sets)))
        self.extra_count = len(sets)

    @property
    def extra_bands(self):
        arr = (Bands * RO_MAX_EXTRA_BANDS)()
        n = library().ro_stft_extra_bands(self._h, arr)
        if n < 0:
            _check(n)
        return [arr[i] for i in range(n)]

    # -- resident path
    def run_resident_sets(self, d_iq, fmt, samples, first_row, rows, d_rows, row_stride=None, d_tile=None,
                          d_records=None, d_extra=None, stream=None):
        """run_resident + d_extra: rows x extra_count records, set s of row r at [r * extra_count + s]"""
        _check(library().ro_stft_run_resident_sets(self._h, _ptr(d_iq), fmt, samples, first_row, rows,
                                                   _ptr(d_rows), row_stride or self.bins, _ptr(d_tile),
                                                   _ptr(d_records), _ptr(d_extra), _ptr(stream)))

    def events_resident(self, rows, detectors, d_state, d_records=None, d_extra=None, first_row=0, d_events=None,
                        capacity=0, d_summary=None, d_detect=None, stream=None):
        """events from scan records that are in HBM, for the primary (d_records: slot 0) and the extra sets (d_extra: slots
        1 + s) at once -- ro_stft_events_resident.  detectors: 1 + extra_count of Detector or (advance, jitter); d_state:
        1 + extra_count DETECT_STATE_DTYPE entries, zero-filled once; d_events: [slot][capacity] EVENT_DTYPE; d_summary:
        1 + extra_count DETECT_SUMMARY_DTYPE; d_detect: [row][1 + extra_count] bytes"""
        if len(detectors) != 1 + self.extra_count:
            raise ValueError("detectors: one per slot, %d" % (1 + self.extra_count))
        _check(library().ro_stft_events_resident(self._h, _ptr(d_records), _ptr(d_extra), first_row, rows,
                                                 _detectors(detectors), _ptr(d_state), _ptr(d_events), capacity,
                                                 _ptr(d_summary), _ptr(d_detect), _ptr(stream)))

    def run_resident_events(self, d_iq, fmt, samples, first_row, rows, d_rows, detectors, d_state, row_stride=None,
                            d_tile=None, d_records=None, d_extra=None, d_events=None, capacity=0, d_summary=None,
                            d_detect=None, stream=None):
        """run_resident_sets, then events_resident on the records it has just written, on the same stream: samples in,
        events out -- ro_stft_run_resident_events"""
        if len(detectors) != 1 + self.extra_count:
            raise ValueError("detectors: one per slot, %d" % (1 + self.extra_count))
        _check(library().ro_stft_run_resident_events(self._h, _ptr(d_iq), fmt, samples, first_row, rows, _ptr(d_rows),
                                                     row_stride or self.bins, _ptr(d_tile), _ptr(d_records),
                                                     _ptr(d_extra), _detectors(detectors), _ptr(d_state), _ptr(d_events),
                                                     capacity, _ptr(d_summary), _ptr(d_detect), _ptr(stream)))

    def ring_put_resident(self, d_image, first_row, rows, ring, image_stride=None, stream=None):
        """rows of d_image (rows x image_stride floats; None: the ring's cols) into the ring's slots: image row i is stream
        row first_row + i and goes to slot (first_row + i) % ring_rows -- ro_stft_ring_put_resident.  ring: RowRing"""
        _check(library().ro_stft_ring_put_resident(self._h, _ptr(d_image), ring.cols if image_stride is None else image_stride,
                                                   first_row, rows, C.byref(ring), _ptr(stream)))

    def snapshots_resident(self, slot_mask, snapshot_rows, ring, head_row, d_pending, d_pending_count, pending_capacity,
                           d_dir, d_arena, arena_floats, d_snap_summary, d_events=None, capacity=0, d_summary=None,
                           stream=None):
        """the rows of every complete event's snapshot out of the ring into d_arena, with a directory; the incomplete ones
        are carried in d_pending from call to call -- ro_stft_snapshots_resident.  d_events [slot][capacity] (EVENT_DTYPE)
        and d_summary [slot] as events_resident leaves them; snapshot_rows: one int per slot up to the mask's highest bit,
        or one for all; d_pending [slots][pending_capacity] events and d_pending_count [slots] int64, zero-filled once;
        d_dir: slots x (capacity + pending_capacity) SNAPSHOT_DTYPE entries; d_snap_summary: one SNAP_SUMMARY_DTYPE"""
        rows_arr, _ = _snapshot_rows(snapshot_rows, slot_mask)
        _check(library().ro_stft_snapshots_resident(self._h, _ptr(d_events), capacity, _ptr(d_summary), slot_mask, rows_arr,
                                                    C.byref(ring), head_row, _ptr(d_pending), _ptr(d_pending_count),
                                                    pending_capacity, _ptr(d_dir), _ptr(d_arena), arena_floats,
                                                    _ptr(d_snap_summary), _ptr(stream)))

    def raw_resident(self, d_dir, dir_capacity, d_snap_summary, spans, d_pending, d_pending_count, pending_capacity,
                     d_raw_dir, d_arena, arena_floats, d_raw_summary, stream=None):
        """the I/Q samples behind every captured snapshot of d_dir, cut out of the sample buffers `spans` names and packed as
        (float)re, (float)im pairs into d_arena, with a directory; the runs whose samples have not all arrived are carried
        in d_pending from call to call -- ro_stft_raw_resident.  d_dir [dir_capacity] (SNAPSHOT_DTYPE) and d_snap_summary
        as snapshots_resident leaves them; spans: up to RO_MAX_IQ_SPANS of IqSpan or (d_iq, first_sample, samples, format),
        ascending, without a gap; d_pending [pending_capacity] SNAPSHOT_DTYPE and d_pending_count, one int64, zero-filled
        once; d_raw_dir: pending_capacity + dir_capacity RAW_CAPTURE_DTYPE entries; d_raw_summary: one RAW_SUMMARY_DTYPE"""
        arr, count = _spans(spans)
        _check(library().ro_stft_raw_resident(self._h, _ptr(d_dir), dir_capacity, _ptr(d_snap_summary), arr, count,
                                              _ptr(d_pending), _ptr(d_pending_count), pending_capacity, _ptr(d_raw_dir),
                                              _ptr(d_arena), arena_floats, _ptr(d_raw_summary), _ptr(stream)))

    def snapshot_units_resident(self, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows,
                                d_unit_dir, d_units, units_bytes, d_unit_summary, stream=None):
        """the FITS data unit of every captured image of d_dir: cut to its slot's columns, big-endian, zero-padded to 2880
        bytes, packed into d_units with a directory -- ro_stft_snapshot_units_resident.  d_dir [dir_capacity]
        (SNAPSHOT_DTYPE), d_snap_summary and d_arena (rows of `cols` floats) as snapshots_resident leaves them;
        slot_windows: (first_col, cols) of each slot's recorder in the image, None: not wanted; d_unit_dir: dir_capacity
        FITS_UNIT_DTYPE entries; d_units: units_bytes bytes, aligned to 16; d_unit_summary: one UNIT_SUMMARY_DTYPE"""
        _check(library().ro_stft_snapshot_units_resident(self._h, _ptr(d_dir), dir_capacity, _ptr(d_snap_summary), _ptr(d_arena),
                                                         arena_floats, cols, _slot_windows(slot_windows), _ptr(d_unit_dir),
                                                         _ptr(d_units), units_bytes, _ptr(d_unit_summary), _ptr(stream)))

    def raw_units_resident(self, d_raw_dir, dir_capacity, d_raw_summary, d_arena, arena_floats, d_unit_dir, d_units,
                           units_bytes, d_unit_summary, stream=None):
        """the FITS data unit (2 x samples) of every captured run of d_raw_dir -- ro_stft_raw_units_resident.  d_raw_dir
        [dir_capacity] (RAW_CAPTURE_DTYPE), d_raw_summary and d_arena as raw_resident leaves them; the outputs as
        snapshot_units_resident takes them"""
        _check(library().ro_stft_raw_units_resident(self._h, _ptr(d_raw_dir), dir_capacity, _ptr(d_raw_summary), _ptr(d_arena),
                                                    arena_floats, _ptr(d_unit_dir), _ptr(d_units), units_bytes,
                                                    _ptr(d_unit_summary), _ptr(stream)))

    def periodic_units_resident(self, ring, recorders, directory, d_units, units_bytes, stream=None):
        """the FITS data unit of every WRITTEN entry of `directory`, cut from the ring's slots to its recorder's columns,
        big-endian, zero-padded to 2880 bytes, at the entry's offset of d_units: one launch --
        ro_stft_periodic_units_resident.  ring: RowRing; recorders and directory (HOST, PERIODIC_ENTRY_DTYPE) as
        periodic_plan took and returned them; d_units: units_bytes bytes, aligned to 16.  Issue it behind ring_put_resident
        on the same stream"""
        recs = periodic_recorders(recorders)
        directory = np.ascontiguousarray(directory)
        if directory.dtype != PERIODIC_ENTRY_DTYPE or directory.ndim != 1:
            raise ValueError("directory: PERIODIC_ENTRY_DTYPE [entries]")
        p = lambda a: C.c_void_p(a.ctypes.data)
        _check(library().ro_stft_periodic_units_resident(self._h, C.byref(ring), p(recs) if len(recs) else None, len(recs),
                                                         p(directory) if len(directory) else None, len(directory),
                                                         _ptr(d_units), units_bytes, _ptr(stream)))

    def snapshot_levels_resident(self, d_dir, dir_capacity, d_snap_summary, d_arena, arena_floats, cols, slot_windows,
                                 d_level_dir, d_ranges, d_levels, levels_bytes, d_level_summary, stream=None):
        """the grey-level preview of every captured image of d_dir: the viewer's ln image of its slot's columns as one byte
        per pixel, zero-padded to 720 bytes, packed into d_levels with a directory and each image's range --
        ro_stft_snapshot_levels_resident.  The sources as snapshot_units_resident takes them; d_level_dir: dir_capacity
        FITS_UNIT_DTYPE entries (level terms); d_ranges: dir_capacity LEVEL_RANGE_DTYPE entries; d_levels: levels_bytes
        bytes, aligned to 16; d_level_summary: one UNIT_SUMMARY_DTYPE"""
        _check(library().ro_stft_snapshot_levels_resident(self._h, _ptr(d_dir), dir_capacity, _ptr(d_snap_summary), _ptr(d_arena),
                                                          arena_floats, cols, _slot_windows(slot_windows), _ptr(d_level_dir),
                                                          _ptr(d_ranges), _ptr(d_levels), levels_bytes, _ptr(d_level_summary),
                                                          _ptr(stream)))

    def periodic_levels_resident(self, ring, recorders, directory, d_ranges, d_levels, levels_bytes, stream=None):
        """the grey-level preview of every WRITTEN entry of `directory`, cut from the ring's slots to its recorder's
        columns, at a quarter of the entry's offset of d_levels, its range at d_ranges[entry]: three launches --
        ro_stft_periodic_levels_resident.  ring, recorders and directory (HOST) as periodic_units_resident takes them;
        d_ranges: len(directory) LEVEL_RANGE_DTYPE entries; d_levels: levels_bytes bytes, aligned to 16"""
        recs = periodic_recorders(recorders)
        directory = np.ascontiguousarray(directory)
        if directory.dtype != PERIODIC_ENTRY_DTYPE or directory.ndim != 1:
            raise ValueError("directory: PERIODIC_ENTRY_DTYPE [entries]")
        p = lambda a: C.c_void_p(a.ctypes.data)
        _check(library().ro_stft_periodic_levels_resident(self._h, C.byref(ring), p(recs) if len(recs) else None, len(recs),
                                                          p(directory) if len(directory) else None, len(directory),
                                                          _ptr(d_ranges), _ptr(d_levels), levels_bytes, _ptr(stream)))

    def levels_png_resident(self, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png,
                            png_bytes, d_png_summary, stream=None):
        """Every level image of a level directory as a complete PNG (8 bit grey, stored deflate blocks), each at a multiple
        of 16 bytes of d_png, with a directory -- ro_stft_levels_png_resident.  d_level_dir / d_level_summary / d_levels as
        snapshot_levels_resident left them (or the upload of periodic_level_dir); d_png_dir: dir_capacity FITS_UNIT_DTYPE
        entries; d_png: png_bytes bytes, aligned to 16; d_png_summary: one UNIT_SUMMARY_DTYPE entry"""
        _check(library().ro_stft_levels_png_resident(self._h, _ptr(d_level_dir), dir_capacity, _ptr(d_level_summary),
                                                     _ptr(d_levels), levels_bytes, _ptr(d_png_dir), _ptr(d_png), png_bytes,
                                                     _ptr(d_png_summary), _ptr(stream)))

    def levels_png_deflate_resident(self, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png,
                                    png_bytes, d_png_summary, stream=None):
        """levels_png_resident with the files' deflate blocks Huffman coded where that is shorter --
        ro_stft_levels_png_deflate_resident.  The files are packed by their actual sizes, at most png_bytes(naxis1, naxis2)
        each; d_png = None with png_bytes = 0 is the sizing call (d_png_summary's needed_bytes)"""
        _check(library().ro_stft_levels_png_deflate_resident(self._h, _ptr(d_level_dir), dir_capacity, _ptr(d_level_summary),
                                                             _ptr(d_levels), levels_bytes, _ptr(d_png_dir), _ptr(d_png),
                                                             png_bytes, _ptr(d_png_summary), _ptr(stream)))

    def levels_resize_resident(self, info, d_plan, d_levels, levels_bytes, d_out_levels, out_levels_bytes, stream=None):
        """Every level image a resize plan has a job for, resized as fits2png's --width does (Pillow's Lanczos, to the byte),
        at its out entry's offset of d_out_levels: two launches -- ro_stft_levels_resize_resident.  info: what resize_plan
        returned (HOST); d_plan: the upload of its blob, on the same stream; d_levels / d_out_levels: aligned to 16.  The out
        directory and summary are resize_plan's: upload them for levels_png_resident"""
        info = np.ascontiguousarray(info).reshape(-1)
        if info.dtype != RESIZE_INFO_DTYPE or info.size < 1:
            raise ValueError("info: RESIZE_INFO_DTYPE")
        _check(library().ro_stft_levels_resize_resident(self._h, C.c_void_p(info.ctypes.data), _ptr(d_plan), _ptr(d_levels),
                                                        levels_bytes, _ptr(d_out_levels), out_levels_bytes, _ptr(stream)))

    def scan_sets_resident(self, d_rows, rows, d_extra, d_records=None, row_stride=None, stream=None):
        """scan_resident for the extra sets (and the primary too when d_records is given)"""
        _check(library().ro_stft_scan_sets_resident(self._h, _ptr(d_rows), row_stride or self.bins, rows,
                                                    _ptr(d_records), _ptr(d_extra), _ptr(stream)))

    def run_resident(self, d_iq, fmt, samples, first_row, rows, d_rows, row_stride=None, d_tile=None,
                     d_records=None, stream=None):
        _check(library().ro_stft_run_resident(self._h, _ptr(d_iq), fmt, samples, first_row, rows,
                                              _ptr(d_rows), row_stride or self.bins, _ptr(d_tile),
                                              _ptr(d_records), _ptr(stream)))

    def run_resident_ln(self, d_iq, fmt, samples, first_row, rows, d_rows, d_tile, d_ln=None, d_minmax=None,
                        row_stride=None, d_records=None, stream=None):
        """run_resident + the log of the tile and the rows' min / max of it (handle created with tile_ln=True)"""
        _check(library().ro_stft_run_resident_ln(self._h, _ptr(d_iq), fmt, samples, first_row, rows, _ptr(d_rows),
                                                 row_stride or self.bins, _ptr(d_tile), _ptr(d_ln), _ptr(d_minmax),
                                                 _ptr(d_records), _ptr(stream)))

    def fetch_ln(self, max_rows):
        """(first_row, tile, ln, minmax[rows, 2], records or None) of up to max_rows rows (tile_ln handles)"""
        cols = self.tile[1]
        tile = np.empty((max_rows, cols), np.float32)
        ln = np.empty((max_rows, cols), np.float32)
        mm = np.empty((max_rows, 2), np.float32)
        recs = np.empty(max_rows, dtype=SCAN_DTYPE) if self.scan_enabled else None
        first, got = C.c_int64(), C.c_int64()
        _check(library().ro_stft_fetch_ln(self._h, max_rows, C.c_void_p(tile.ctypes.data), C.c_void_p(ln.ctypes.data),
                                          C.c_void_p(mm.ctypes.data),
                                          C.c_void_p(recs.ctypes.data) if recs is not None else None,
                                          C.byref(first), C.byref(got)))
        g = got.value
        return first.value, tile[:g], ln[:g], mm[:g], (recs[:g] if recs is not None else None)

    def spectra_resident(self, d_iq, fmt, samples, first_row, rows, d_spectra, stride=None, stream=None):
        """complex spectra (rows x stride x {re, im} float32, bin k at element k) instead of magnitudes"""
        _check(library().ro_stft_spectra_resident(self._h, _ptr(d_iq), fmt, samples, first_row, rows,
                                                  _ptr(d_spectra), stride or self.bins, _ptr(stream)))

    def band_resident(self, d_iq, fmt, samples, first_row, rows, first_col, cols, d_band, band_stride=None,
                      d_records=None, stream=None):
        """columns [first_col, +cols) of the rows and nothing else (rows x band_stride float32), plus their scan records"""
        _check(library().ro_stft_band_resident(self._h, _ptr(d_iq), fmt, samples, first_row, rows, first_col, cols,
                                               _ptr(d_band), band_stride or cols, _ptr(d_records), _ptr(stream)))

    def band_windows_resident(self, d_iq, fmt, samples, first_row, rows, windows, d_band, band_stride=None,
                              d_records=None, d_extra=None, stream=None):
        """the columns of `windows` (BandWindow or (first_col, cols) each, ascending) side by side in rows x band_stride
        float32 and nothing else, plus the scan records of the primary (d_records) and the extra sets (d_extra)"""
        arr, n = _windows(windows)
        total = sum(arr[i].cols for i in range(n))
        _check(library().ro_stft_band_windows_resident(self._h, _ptr(d_iq), fmt, samples, first_row, rows, arr, n,
                                                       _ptr(d_band), band_stride or total, _ptr(d_records),
                                                       _ptr(d_extra), _ptr(stream)))

    def cut_windows_resident(self, d_rows, rows, windows, d_image, row_stride=None, image_stride=None, stream=None):
        """the columns of `windows` (BandWindow or (first_col, cols) each, ascending) of rows already in HBM, side by
        side in rows x image_stride float32 -- ro_stft_cut_windows_resident"""
        arr, n = _windows(windows)
        total = sum(arr[i].cols for i in range(n))
        _check(library().ro_stft_cut_windows_resident(self._h, _ptr(d_rows), row_stride or self.bins, rows, arr, n,
                                                      _ptr(d_image), image_stride or total, _ptr(stream)))

    def run_resident_windows(self, d_iq, fmt, samples, first_row, rows, d_rows, windows, d_image, row_stride=None,
                             image_stride=None, d_records=None, d_extra=None, stream=None):
        """run_resident_sets without a tile, then the columns of `windows` of those rows side by side in rows x
        image_stride float32; the records are the full rows', in row coordinates -- ro_stft_run_resident_windows"""
        arr, n = _windows(windows)
        total = sum(arr[i].cols for i in range(n))
        _check(library().ro_stft_run_resident_windows(self._h, _ptr(d_iq), fmt, samples, first_row, rows, _ptr(d_rows),
                                                      row_stride or self.bins, arr, n, _ptr(d_image),
                                                      image_stride or total, _ptr(d_records), _ptr(d_extra),
                                                      _ptr(stream)))

    def scan_resident(self, d_rows, rows, d_records, row_stride=None, stream=None):
        _check(library().ro_stft_scan_resident(self._h, _ptr(d_rows), row_stride or self.bins, rows,
                                               _ptr(d_records), _ptr(stream)))

    def ln_tile_resident(self, d_rows, rows, first_col, cols, d_ln=None, d_u8=None, d_minmax=None,
                         row_stride=None, stream=None):
        _check(library().ro_stft_ln_tile_resident(self._h, _ptr(d_rows), row_stride or self.bins, rows, first_col,
                                                  cols, _ptr(d_ln), _ptr(d_u8), _ptr(d_minmax), _ptr(stream)))

    def time_resident(self, d_iq, fmt, samples, first_row, rows, d_rows, iters, row_stride=None,
                      d_tile=None, d_records=None, stream=None):
        ms = (C.c_float * iters)()
        kern = (C.c_float * 2)()
        _check(library().ro_stft_time_resident(self._h, _ptr(d_iq), fmt, samples, first_row, rows,
                                               _ptr(d_rows), row_stride or self.bins, _ptr(d_tile),
                                               _ptr(d_records), _ptr(stream), iters, ms, kern))
        return np.array(ms[:], dtype=np.float64), float(kern[0]), float(kern[1])

    # -- streaming path
    def push(self, iq):
        """iq: numpy array, complex64 / complex128 / float32 [n,2] / float64 [n,2] / int16 [n,2]."""
        a = np.ascontiguousarray(iq)
        if a.dtype == np.complex64:
            a, fmt = a.view(np.float32), RO_IQ_F32
        elif a.dtype == np.complex128:
            a, fmt = a.view(np.float64), RO_IQ_F64
        elif a.dtype == np.float32:
            fmt = RO_IQ_F32
        elif a.dtype == np.float64:
            fmt = RO_IQ_F64
        elif a.dtype == np.int16:
            fmt = RO_IQ_I16
        else:
            raise TypeError("unsupported sample dtype %s" % a.dtype)
        n = a.size // 2
        ready = C.c_int64()
        _check(library().ro_stft_push(self._h, C.c_void_p(a.ctypes.data), fmt, n, C.byref(ready)))
        return ready.value

    def flush(self):
        ready = C.c_int64()
        _check(library().ro_stft_flush(self._h, C.byref(ready)))
        return ready.value

    def set_tile_windows(self, windows):
        """up to RO_MAX_TILE_WINDOWS column windows (BandWindow or (first_col, cols) each, ascending) cut from every
        row of the streaming path: only their image travels to the host, and fetch / fetch_sets count in image columns;
        an empty list restores full rows -- ro_stft_set_tile_windows"""
        arr, n = _windows(windows or [])
        _check(library().ro_stft_set_tile_windows(self._h, arr, n))
        self.image_cols = sum(arr[i].cols for i in range(n))

    @property
    def tile_windows(self):
        arr = (BandWindow * RO_MAX_TILE_WINDOWS)()
        n = library().ro_stft_tile_windows(self._h, arr)
        if n < 0:
            _check(n)
        return [BandWindow(arr[i].first_col, arr[i].cols) for i in range(n)]

    def _default_columns(self, first_col, cols):
        """everything this handle brings to the host: the tile windows' image, the tile, or the full row"""
        lo, n = (0, self.image_cols) if self.image_cols else self.tile if self.tile else (0, self.bins)
        if first_col is None:
            first_col = lo
        if cols is None:
            cols = lo + n - first_col
        return first_col, cols

    def fetch(self, max_rows, first_col=None, cols=None, want_records=None):
        first_col, cols = self._default_columns(first_col, cols)
        want_records = self.scan_enabled if want_records is None else want_records
        rows = np.empty((max_rows, cols), dtype=np.float32)
        recs = np.empty(max_rows, dtype=SCAN_DTYPE) if want_records else None
        first = C.c_int64()
        got = C.c_int64()
        _check(library().ro_stft_fetch(
            self._h, max_rows, first_col, cols, rows.ctypes.data_as(C.POINTER(C.c_float)),
            recs.ctypes.data_as(C.POINTER(ScanRecord)) if recs is not None else None,
            C.byref(first), C.byref(got)))
        g = got.value
        return first.value, rows[:g], (recs[:g] if recs is not None else None)

    def fetch_sets(self, max_rows, first_col=None, cols=None, want_rows=None, want_extra=True):
        """ro_stft_fetch_sets: (first_row_index, rows, records, extra) with extra shaped (rows_got, extra_count); rows is
        None for a handle with a row sink (they are in the ring), records None without a primary set"""
        first_col, cols = self._default_columns(first_col, cols)
        want_rows = (getattr(self, "_sink", None) is None) if want_rows is None else want_rows
        rows = np.empty((max_rows, cols), dtype=np.float32) if want_rows else None
        recs = np.empty(max_rows, dtype=SCAN_DTYPE) if self.scan_enabled else None
        count = self.extra_count
        extra = np.empty((max_rows, max(count, 1)), dtype=SCAN_DTYPE) if want_extra else None
        first, got = C.c_int64(), C.c_int64()
        _check(library().ro_stft_fetch_sets(
            self._h, max_rows, first_col if want_rows else 0, cols if want_rows else 0,
            rows.ctypes.data_as(C.POINTER(C.c_float)) if rows is not None else None,
            recs.ctypes.data_as(C.POINTER(ScanRecord)) if recs is not None else None,
            extra.ctypes.data_as(C.POINTER(ScanRecord)) if extra is not None else None,
            C.byref(first), C.byref(got)))
        g = got.value
        return (first.value, rows[:g] if rows is not None else None, recs[:g] if recs is not None else None,
                extra[:g, :count] if extra is not None else None)

    def reset(self):
        _check(library().ro_stft_reset(self._h))

    def set_row_sink(self, ring, first_slot=0):
        """ring: a C-contiguous float32 numpy array [capacity_rows, row_stride] that stays alive (and unmoved) while it
        is the sink (pinned_array gives page-locked ones); None removes the sink"""
        if ring is None:
            _check(library().ro_stft_set_row_sink(self._h, None, 0, 0, 0))
            self._sink = None
            return
        assert ring.dtype == np.float32 and ring.ndim == 2 and ring.flags["C_CONTIGUOUS"]
        _check(library().ro_stft_set_row_sink(self._h, C.c_void_p(ring.ctypes.data), ring.shape[1], ring.shape[0], first_slot))
        self._sink = ring

    def fetch_records(self, max_rows):
        """ro_stft_fetch with rows_out = NULL (the rows are in the sink): (first row index, rows got, records or None)"""
        recs = np.empty(max_rows, dtype=SCAN_DTYPE) if self.scan_enabled else None
        first, got = C.c_int64(), C.c_int64()
        _check(library().ro_stft_fetch(self._h, max_rows, 0, 0, None,
                                       recs.ctypes.data_as(C.POINTER(ScanRecord)) if recs is not None else None,
                                       C.byref(first), C.byref(got)))
        return first.value, got.value, (recs[:got.value] if recs is not None else None)

    def timing(self, reset=False):
        t = Timing()
        _check(library().ro_stft_timing(self._h, C.byref(t), 1 if reset else 0))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def rows_complete(self):
        """rows ro_stft_fetch would hand over without waiting (their batches have finished on the device)"""
        n = C.c_int64()
        _check(library().ro_stft_rows_complete(self._h, C.byref(n)))
        return n.value

    def stats(self):
        s, r, l = C.c_int64(), C.c_int64(), C.c_int64()
        ms = C.c_double()
        _check(library().ro_stft_stats(self._h, C.byref(s), C.byref(r), C.byref(l), C.byref(ms)))
        return {"samples_in": s.value, "rows_out": r.value, "launches": l.value,
                "kernel_ms_total": ms.value}
