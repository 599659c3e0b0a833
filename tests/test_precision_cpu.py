"""CPU: WaterfallConfig::precision and the "waterfall" factory's key parser (parseWaterfallKeys,
radio-observer_amd/host/HipWaterfallBackend.h) through the test-only shim tests/harness_precision/."""
import ctypes as C

import pytest

import precisionlib as P


@pytest.fixture(autouse=True)
def _need_shim():
    assert P.precision_library() is not None, "tests/harness_precision/libro_precision_harness.so missing: run build()"


def test_shim_exports_what_the_wrapper_binds():
    L = C.CDLL(P.PATH)
    for name, _, _ in P.SIGNATURES:
        assert hasattr(L, name), name


def test_defaults_are_the_reference_factory_defaults_and_f32():
    """WaterfallBackend::make's defaults (src/WaterfallBackend.cpp:620-646) and float32: every existing caller is
    unchanged."""
    assert P.precision_library().ro_prec_default_precision() == P.RO_PRECISION_F32
    ok, cfg, err = P.parse_keys({})
    assert ok and err == ""
    assert cfg == dict(bins=32768, overlap=0, buffer_chunk_size=1024 * 1024, iq_phase_shift=0,
                       precision=P.RO_PRECISION_F32, iq_gain=0.0, origin="debug", metadata_path=".")


def test_every_key():
    ok, cfg, err = P.parse_keys({"bins": "65536", "overlap": "49152", "origin": "svakov", "metadata_path": "/data/meta",
                                 "buffer_chunk_size": "2097152", "iq_gain": "-0.25", "iq_phase_shift": "3",
                                 "precision": "f64", "unrelated": "kept out"})
    assert ok, err
    assert cfg == dict(bins=65536, overlap=49152, buffer_chunk_size=2097152, iq_phase_shift=3,
                       precision=P.RO_PRECISION_F64, iq_gain=-0.25, origin="svakov", metadata_path="/data/meta")


@pytest.mark.parametrize("value,want", [("f32", P.RO_PRECISION_F32), ("f64", P.RO_PRECISION_F64)])
def test_precision_values(value, want):
    ok, cfg, err = P.parse_keys({"precision": value})
    assert ok and err == "" and cfg["precision"] == want


@pytest.mark.parametrize("value", ["double", "F64", "fp64", "64", "", " f64", "f64 "])
def test_unknown_precision_is_refused_with_text(value):
    ok, cfg, err = P.parse_keys({"bins": "1024", "precision": value})
    assert not ok
    assert "precision" in err and repr(value)[1:-1] in err and "f32" in err and "f64" in err
    assert cfg["bins"] == 32768 and cfg["precision"] == P.RO_PRECISION_F32     # nothing half-applied


@pytest.mark.parametrize("key,value", [("bins", "32k"), ("overlap", ""), ("iq_gain", "0.5x"),
                                       ("buffer_chunk_size", "99999999999"), ("iq_phase_shift", "1.5")])
def test_malformed_numbers_are_refused(key, value):
    ok, cfg, err = P.parse_keys({key: value, "precision": "f64"})
    assert not ok and key in err
    assert cfg["precision"] == P.RO_PRECISION_F32
