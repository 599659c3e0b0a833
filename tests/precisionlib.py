"""ctypes access to WaterfallConfig::precision and the "waterfall" factory's key parser of the product's host-side C++
mirror (radio-observer_amd/host/libro_host.so) through the test-only shim tests/harness_precision/
libro_precision_harness.so, which links it.  precision_library() returns None when the shim has not been built."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "harness_precision", "libro_precision_harness.so")
RO_PRECISION_F32, RO_PRECISION_F64 = 0, 1          # include/ro_stft.h
_lib = False


class BolidEvent(C.Structure):                      # radio-observer_amd/host/BolidRecorder.h
    _fields_ = [("row", C.c_int64), ("start", C.c_int), ("length", C.c_int), ("duration", C.c_float),
                ("noise", C.c_float), ("peakFreq", C.c_float), ("magnitude", C.c_float), ("fmin", C.c_float),
                ("fmax", C.c_float), ("rawLength", C.c_int)]


_VP, _I, _I64, _F, _D, _S = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_char_p
# every symbol this module binds: (name, restype, argtypes)
SIGNATURES = [
    ("ro_prec_parse_keys", _I, [_S, C.POINTER(_I), C.POINTER(_D), _S, _I, _S, _I, _S, _I]),
    ("ro_prec_default_precision", _I, []),
    ("ro_prec_pipeline_create", _VP, [_I, _I, _I, _I, _I64, _I64, _I, _I, _F, _F, _F, _F, _D, _D, _F, _F, _F, _S, _S]),
    ("ro_prec_pipeline_destroy", None, [_VP]),
    ("ro_prec_pipeline_set_clock", None, [_VP, _I64, _I64]),
    ("ro_prec_pipeline_process", None, [_VP, C.POINTER(_D), _I]),
    ("ro_prec_pipeline_end", None, [_VP]),
    ("ro_prec_pipeline_rows", _I64, [_VP]),
    ("ro_prec_pipeline_error", _S, [_VP]),
    ("ro_prec_pipeline_precision", _I, [_VP]),
    ("ro_prec_pipeline_ring_capacity", _I, [_VP]),
    ("ro_prec_pipeline_ring_mark", _I, [_VP]),
    ("ro_prec_pipeline_raw_capacity", _I, [_VP]),
    ("ro_prec_pipeline_raw_mark", _I, [_VP]),
    ("ro_prec_pipeline_batch_rows", _I, [_VP]),
    ("ro_prec_pipeline_state", _I, [_VP]),
    ("ro_prec_pipeline_ring_row", None, [_VP, _I, C.POINTER(_F)]),
    ("ro_prec_pipeline_raw_ring", _I, [_VP, C.POINTER(_F), _I]),
    ("ro_prec_pipeline_row_info", _I, [_VP, _I64, C.POINTER(C.c_uint64), C.POINTER(_I64), C.POINTER(_I64),
                                       C.POINTER(_I)]),
    ("ro_prec_pipeline_raw_handle", None, [_VP, _I, C.POINTER(_I), C.POINTER(_I64), C.POINTER(_I64)]),
    ("ro_prec_pipeline_bands", None, [_VP, C.POINTER(_I)]),
    ("ro_prec_pipeline_events", _I, [_VP, C.POINTER(BolidEvent), _I]),
    ("ro_prec_pipeline_files", _I, [_VP, _I, _S, _I]),
    ("ro_prec_pipeline_timing", _I, [_VP, C.POINTER(_D)]),
    ("ro_prec_wav_to_fits", _I64, [_I, _S, _I64, _I, _I, _I, _I, _F, _F, _S, _S, _I64, _S, _I, _S, _I]),
    ("ro_prec_stream_bench", _I, [_I, _I, _I, _I, _I, _D, _I, _I, C.POINTER(_D)]),
]


def precision_library():
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
    L = precision_library()
    assert L is not None, "%s missing: run __graft_entry__.build()" % PATH
    return L


def parse_keys(keys):
    """parseWaterfallKeys over a dict of strings: (ok, config dict, error text)"""
    L = require()
    text = "".join("%s=%s\n" % (k, v) for k, v in keys.items()).encode()
    i5, gain = (C.c_int * 5)(), C.c_double()
    origin, meta, err = C.create_string_buffer(4096), C.create_string_buffer(4096), C.create_string_buffer(4096)
    ok = L.ro_prec_parse_keys(text, i5, C.byref(gain), origin, 4096, meta, 4096, err, 4096)
    cfg = dict(bins=i5[0], overlap=i5[1], buffer_chunk_size=i5[2], iq_phase_shift=i5[3], precision=i5[4],
               iq_gain=gain.value, origin=origin.value.decode(), metadata_path=meta.value.decode())
    return bool(ok), cfg, err.value.decode()


class PrecisionPipeline:
    """Frontend -> HipWaterfallBackend(precision) -> [SnapshotRecorder] -> BolidRecorder of the host mirror."""

    def __init__(self, bins, overlap, precision, sample_rate=48000, start=(0, 0), max_batch_rows=0,
                 snapshot_length=60, detect=(10300.0, 10900.0), noise=(9000.0, 9600.0), advance_time=2.0,
                 jitter_time=5.0, avg_range=40.0, out_dir=None, origin="teststn", snap_band=(9000.0, 12000.0)):
        self.L = require()
        self.bins = bins
        self.h = self.L.ro_prec_pipeline_create(precision, bins, overlap, sample_rate, start[0], start[1],
                                                max_batch_rows, snapshot_length, detect[0], detect[1], noise[0],
                                                noise[1], advance_time, jitter_time, avg_range, snap_band[0],
                                                snap_band[1], None if out_dir is None else str(out_dir).encode(),
                                                origin.encode())

    def __getattr__(self, name):                     # the int-valued accessors
        if name.startswith("_") or name in ("L", "h", "bins"):
            raise AttributeError(name)
        fn = getattr(self.L, "ro_prec_pipeline_" + name)
        return lambda: fn(self.h)

    def set_clock(self, sec, usec=0):
        self.L.ro_prec_pipeline_set_clock(self.h, sec, usec)

    def process(self, z):
        a = np.ascontiguousarray(z, dtype=np.complex128).view(np.float64)
        self.L.ro_prec_pipeline_process(self.h, a.ctypes.data_as(C.POINTER(C.c_double)), a.size // 2)

    def end(self):
        self.L.ro_prec_pipeline_end(self.h)

    @property
    def rows(self):
        return self.L.ro_prec_pipeline_rows(self.h)

    @property
    def error(self):
        return (self.L.ro_prec_pipeline_error(self.h) or b"").decode()

    def ring_row(self, mark):
        out = np.empty(self.bins, np.float32)
        self.L.ro_prec_pipeline_ring_row(self.h, mark, out.ctypes.data_as(C.POINTER(C.c_float)))
        return out

    def newest_rows(self, n):
        m = self.ring_mark()
        return np.stack([self.ring_row(m - n + i) for i in range(n)])

    def raw_ring(self):
        cap = self.L.ro_prec_pipeline_raw_ring(self.h, None, 0)
        out = np.empty((cap, 2), np.float32)
        self.L.ro_prec_pipeline_raw_ring(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), cap)
        return out

    def row_info(self, i):
        o, s, u, m = C.c_uint64(), C.c_int64(), C.c_int64(), C.c_int()
        assert self.L.ro_prec_pipeline_row_info(self.h, i, C.byref(o), C.byref(s), C.byref(u), C.byref(m)) == 0
        return (o.value, s.value, u.value, m.value)

    def raw_handle(self, mark):
        m, s, u = C.c_int(), C.c_int64(), C.c_int64()
        self.L.ro_prec_pipeline_raw_handle(self.h, mark, C.byref(m), C.byref(s), C.byref(u))
        return (m.value, s.value, u.value)

    def bands(self):
        out = (C.c_int * 7)()
        self.L.ro_prec_pipeline_bands(self.h, out)
        return list(out)

    def events(self):
        buf = (BolidEvent * 256)()
        n = self.L.ro_prec_pipeline_events(self.h, buf, 256)
        return [buf[i] for i in range(min(n, 256))]

    def files(self, kind):
        """kind 0: the SnapshotRecorder's FITS files, 1: the detector's band snapshots, 2: its raw I/Q captures"""
        buf = C.create_string_buffer(1 << 16)
        self.L.ro_prec_pipeline_files(self.h, kind, buf, 1 << 16)
        return buf.value.decode().split()

    def timing(self):
        out = (C.c_double * 6)()
        assert self.L.ro_prec_pipeline_timing(self.h, out) == 0
        return dict(push_calls=out[0], push_ms_avg=out[1], batches=out[2], batch_gpu_ms_avg=out[3],
                    fetch_calls=out[4], fetch_ms_avg=out[5])

    def close(self):
        if self.h:
            self.L.ro_prec_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def wav_to_fits(precision, payload, bins, overlap, max_batch_rows, snapshot_length, lo, hi, out_dir, origin,
                clock_sec=-1):
    """C1: WAV bytes -> WAVStream -> HipWaterfallBackend(precision) -> SnapshotRecorder -> FITS: (rows, files, error)"""
    L = require()
    files, err = C.create_string_buffer(1 << 16), C.create_string_buffer(4096)
    rows = L.ro_prec_wav_to_fits(precision, payload, len(payload), bins, overlap, max_batch_rows, snapshot_length, lo,
                                 hi, str(out_dir).encode(), origin.encode(), clock_sec, files, 1 << 16, err, 4096)
    return rows, files.value.decode().split(), err.value.decode()


STREAM_STATS = ("seconds", "samples", "rows", "calls", "batch_rows", "call_ms_avg", "call_ms_max", "events",
                "push_ms_avg", "fetch_ms_avg", "batch_gpu_ms_avg", "row_gpu_us_avg", "push_calls", "fetch_calls",
                "batches", "rows_by_dma")


def stream_bench(precision, bins, overlap, sample_rate=48000, block=4096, seconds=3.0, max_batch_rows=0,
                 warm_calls=200):
    """rows/s through Backend::process (ro_prec_stream_bench): (return code, stats dict)"""
    L = require()
    st = (C.c_double * 16)()
    rc = L.ro_prec_stream_bench(precision, bins, overlap, sample_rate, block, seconds, max_batch_rows, warm_calls, st)
    return rc, dict(zip(STREAM_STATS, list(st)))
