"""ctypes access to several BolidRecorders on one waterfall of the product's host-side C++ mirror
(radio-observer_amd/host/libro_host.so) through the test-only shim tests/harness_detectors/libro_detectors_harness.so,
which links it.  detectors_library() returns None when the shim has not been built."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "harness_detectors", "libro_detectors_harness.so")
_lib = False

SCAN_DTYPE = np.dtype([("noise", np.float32), ("peak", np.int32), ("average", np.float32)])   # ro_scan_record_t


class BolidEvent(C.Structure):                      # radio-observer_amd/host/BolidRecorder.h
    _fields_ = [("row", C.c_int64), ("start", C.c_int), ("length", C.c_int), ("duration", C.c_float),
                ("noise", C.c_float), ("peakFreq", C.c_float), ("magnitude", C.c_float), ("fmin", C.c_float),
                ("fmax", C.c_float), ("rawLength", C.c_int)]


_VP, _I, _I64, _F, _D, _S = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p
_FP, _IP = C.POINTER(C.c_float), C.POINTER(C.c_int)
# every symbol this module binds: (name, restype, argtypes)
SIGNATURES = [
    ("ro_det_pipeline_create", _VP, [_I, _I, _I, _I, _I, _I, _FP, _D, _D, _F]),
    ("ro_det_pipeline_destroy", None, [_VP]),
    ("ro_det_pipeline_process", None, [_VP, C.POINTER(_D), _I]),
    ("ro_det_pipeline_end", None, [_VP]),
    ("ro_det_pipeline_rows", _I64, [_VP]),
    ("ro_det_pipeline_error", _S, [_VP]),
    ("ro_det_pipeline_ring_capacity", _I, [_VP]),
    ("ro_det_pipeline_batch_rows", _I, [_VP]),
    ("ro_det_pipeline_state", _I, [_VP, _I]),
    ("ro_det_pipeline_bands", _I, [_VP, _I, _IP]),
    ("ro_det_pipeline_events", _I, [_VP, _I, C.POINTER(BolidEvent), _I]),
    ("ro_det_manual_create", _VP, [_I, _I, _I, _FP, _D, _D, _F]),
    ("ro_det_manual_start", _I, [_VP, _I]),
    ("ro_det_manual_error", _S, [_VP]),
    ("ro_det_manual_scan_enabled", _I, [_VP]),
    ("ro_det_manual_extra_sets", _I, [_VP]),
    ("ro_det_manual_destroy", None, [_VP]),
    ("ro_det_manual_push", None, [_VP, _VP, _I]),
    ("ro_det_manual_push_single", None, [_VP, _F, _I, _F]),
    ("ro_det_manual_end", None, [_VP]),
    ("ro_det_manual_ring_capacity", _I, [_VP]),
    ("ro_det_manual_state", _I, [_VP, _I]),
    ("ro_det_manual_bands", _I, [_VP, _I, _IP]),
    ("ro_det_manual_events", _I, [_VP, _I, C.POINTER(BolidEvent), _I]),
]


def detectors_library():
    global _lib
    if _lib is False:
        _lib = C.CDLL(PATH) if os.path.exists(PATH) else None
        if _lib is not None:
            for name, res, args in SIGNATURES:
                fn = getattr(_lib, name)
                fn.restype = res
                fn.argtypes = args
    return _lib


def require():
    L = detectors_library()
    assert L is not None, "%s missing: run __graft_entry__.build()" % PATH
    return L


def _freqs(detectors):
    """[(low_detect, hi_detect, low_noise, hi_noise), ...] -> float32 [n, 4]"""
    a = np.ascontiguousarray(detectors, dtype=np.float32).reshape(-1, 4)
    return a, a.ctypes.data_as(_FP)


class _Rig:
    """what the pipeline and the manual rig share: per-detector bands, events, state"""
    prefix = None

    def _fn(self, name):
        return getattr(self.L, self.prefix + name)

    def bands(self, i):
        """(low_detect, detect_width, low_noise, noise_width, advance, jitter, avg_bins, scan slot) of detector i"""
        out = (C.c_int * 8)()
        assert self._fn("bands")(self.h, i, out) == 0
        return tuple(out)

    def events(self, i):
        buf = (BolidEvent * 64)()
        n = self._fn("events")(self.h, i, buf, 64)
        assert 0 <= n <= 64, n
        return [buf[k] for k in range(n)]

    def state(self, i):
        return self._fn("state")(self.h, i)

    def ring_capacity(self):
        return self._fn("ring_capacity")(self.h)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DetectorPipeline(_Rig):
    """Frontend -> HipWaterfallBackend -> len(detectors) BolidRecorders, in that order"""
    prefix = "ro_det_pipeline_"

    def __init__(self, bins, overlap, detectors, precision=0, sample_rate=48000, max_batch_rows=0, advance_time=2.0,
                 jitter_time=5.0, avg_range=40.0):
        self.L = require()
        self.n = len(detectors)
        a, p = _freqs(detectors)
        self.h = self.L.ro_det_pipeline_create(precision, bins, overlap, sample_rate, max_batch_rows, self.n, p,
                                               advance_time, jitter_time, avg_range)

    def process(self, z):
        a = np.ascontiguousarray(z, dtype=np.complex128).view(np.float64)
        self.L.ro_det_pipeline_process(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size // 2)

    def end(self):
        self.L.ro_det_pipeline_end(self.h)

    @property
    def rows(self):
        return self.L.ro_det_pipeline_rows(self.h)

    @property
    def error(self):
        return (self.L.ro_det_pipeline_error(self.h) or b"").decode()

    def batch_rows(self):
        return self.L.ro_det_pipeline_batch_rows(self.h)


class ManualDetectors(_Rig):
    """len(detectors) BolidRecorders on a ManualWaterfall, fed one scan record per detector and row"""
    prefix = "ro_det_manual_"

    def __init__(self, bins, overlap, detectors, sample_rate=48000, advance_time=2.0, jitter_time=5.0, avg_range=40.0):
        self.L = require()
        self.n = len(detectors)
        a, p = _freqs(detectors)
        self.h = self.L.ro_det_manual_create(bins, overlap, self.n, p, advance_time, jitter_time, avg_range)
        self.started = bool(self.L.ro_det_manual_start(self.h, sample_rate))

    @property
    def error(self):
        return (self.L.ro_det_manual_error(self.h) or b"").decode()

    def scan_enabled(self):
        return bool(self.L.ro_det_manual_scan_enabled(self.h))

    def extra_sets(self):
        return self.L.ro_det_manual_extra_sets(self.h)

    def push(self, records):
        """records: one (noise, peak, average) per scan slot, slot 0 first"""
        r = np.array([tuple(x) for x in records], dtype=SCAN_DTYPE)
        self.L.ro_det_manual_push(self.h, r.ctypes.data, len(r))

    def push_single(self, noise, peak, average):
        """the pushRow signature with one record per row"""
        self.L.ro_det_manual_push_single(self.h, noise, peak, average)

    def end(self):
        self.L.ro_det_manual_end(self.h)
