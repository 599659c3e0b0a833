"""GPU: bench.py itself, run in this process (a child process would have to be started from a process that already
holds the GPU): the line carries what the contract asks for, and --workload c5's hash of the stitched band + records
is the hash of the same stream transformed directly through the C ABI."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(argv):
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    sys.argv = ["bench.py"] + argv
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        sys.argv = old
        bench.BINS, bench.OVERLAP, bench.HOP = 32768, 24576, 8192
        bench.ALG_BYTES_PER_ROW = bench.HOP * 8 + bench.BINS * 4
    lines = [l for l in buf.getvalue().splitlines() if l.startswith("{")]
    assert len(lines) == 1, buf.getvalue()[-2000:]
    return json.loads(lines[0])


def test_bench_line_has_the_contract_fields(ro, torch_cuda):
    d = run_bench(["--full", "--steps", "4", "--warmup", "1", "--prewarm", "2", "--rows", "4096", "--cpu-seconds", "1.5",
                   "--stream-seconds", "0.4"])
    assert d["unit"] == "rows/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1 and d["prewarm"] == 2
    assert d["dtype"] == "f32" and d["vs_baseline"] is None and d["scaling"] == "weak"
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and rf["kernel"] == "stft32k_kernel"
    assert rf["achieved"] == pytest.approx(rf["algorithmic_bytes_per_launch"] / (rf["kernel_ms"] * 1e-3) / 1e9)
    assert rf["frac"] == pytest.approx(rf["achieved"] / 8000.0)
    # the kernel's share cannot be below what the whole step makes of the same bytes, nor far from the post-hoc loop
    assert 0 < rf["frac_step"] <= rf["frac"] * 1.001
    assert abs(rf["frac_posthoc"] - rf["frac"]) < 0.35 * rf["frac"]      # (a cold device: a dozen launches in all)
    assert "timed region" in rf["kernel_ms_source"]
    assert d["parity"]["max_err_rel_to_row_max"] <= 1e-5 and d["parity"]["scan_records_bit_exact"]
    sp = d["strict_precision"]
    assert sp["dtype"] == "f64" and sp["parity"]["max_err_per_bin_relative"] <= 1e-5
    assert sp["roofline"]["frac"] == pytest.approx(sp["roofline"]["achieved"] / 8000.0) and "f64r_kernel" in sp["roofline"]["kernel"]
    assert sp["parity"]["max_err_per_bin_relative"] <= 2e-7 and "4096" in sp["c2"]["workload"]
    assert sp["c2"]["dtype"] == "f64" and sp["c2"]["parity"]["max_err_per_bin_relative"] <= 2e-7 and sp["c2"]["value"] > sp["value"]
    assert "1024" in sp["c1"]["workload"] and sp["c1"]["parity"]["max_err_per_bin_relative"] <= 2e-7 and sp["c1"]["value"] > sp["c2"]["value"]
    assert "f64r_kernel" in sp["c1"]["roofline"]["kernel"] and 0 < sp["roofline"]["fp64_valu"]["frac"] < 1
    assert rf["limiter"].startswith("package power cap")
    io = d["ionozor"]                   # the four-step form at Ionozor.json:27-28, never the headline
    assert io["unit"] == "rows/s" and io["value"] > 0 and io["parity"]["max_err_rel_to_row_max"] <= 1e-5
    assert io["roofline"]["frac"] == pytest.approx(io["roofline"]["achieved"] / 8000.0) and "four_cols_kernel" in io["roofline"]["kernel"]
    bo = d["bolidozor"]                 # Bolidozor.json:45-46 on the one-kernel large form
    assert bo["value"] > io["value"] and bo["parity"]["max_err_rel_to_row_max"] <= 1e-5 and "65536" in bo["workload"]
    assert bo["f64"]["dtype"] == "f64" and bo["f64"]["parity"]["max_err_per_bin_relative"] <= 2e-7 and 0 < bo["f64"]["value"] < bo["value"]
    for k in ("streaming", "streaming_batch256"):
        st = d[k]
        assert "error" not in st, st
        assert st["rows"] > 0 and st["samples_per_call"] == 4096 and st["real_time_factor"] > 10
        assert st["value"] == pytest.approx(st["rows"] / st["seconds"])
    assert len(d["config"]["rank0_scan_records_hash"]) == 32          # what an N-rank run's line is compared with
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0
    assert "cpu_baseline_O0" in d and "error" not in d["cpu_baseline_O0"]


def test_bench_plain_run_times_the_steps_and_dumps_what_they_computed(ro, oracle, torch_cuda, tmp_path):
    """a plain run (no --full) is the timed steps and the line; --dump-outputs writes the last step's rows (a fixed
    sample) and scan records, the same from run to run, and they are what the oracle computes from the bench's input"""
    torch = torch_cuda
    R, bins, overlap = 1024, 32768, 24576
    lines = []
    for k in range(2):
        lines.append(run_bench(["--steps", "3", "--warmup", "1", "--prewarm", "1", "--rows", str(R),
                                "--dump-outputs", str(tmp_path / str(k))]))
    d = lines[0]
    assert d["steps"] == 3 and d["full"] is False and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["unit"] == "rows/s" and "N=32768" in d["metric"]
    assert d["value"] * d["ms_per_step"] * 1e-3 == pytest.approx(R)            # R rows in one timed step
    assert d["roofline"]["frac"] == pytest.approx(d["roofline"]["achieved"] / 8000.0)
    for k in ("parity", "strict_precision", "ionozor", "bolidozor", "streaming", "cpu_baseline", "clock_power",
              "device_copy_GBs", "step_ms_back_to_back"):
        assert k not in d, k
    files = sorted(os.listdir(tmp_path / "0"))
    assert files == ["rows.npy", "scan_records.npy"] and sorted(os.listdir(tmp_path / "1")) == files
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in files) <= 64e6
    got = {f: np.load(tmp_path / "0" / f) for f in files}
    for f in files:
        assert np.array_equal(got[f], np.load(tmp_path / "1" / f), equal_nan=True), f
    rows, recs = got["rows.npy"], got["scan_records.npy"]
    assert rows.dtype == np.float32 and rows.shape == (256, bins)               # 32 MiB of the 128 MiB of rows
    assert recs.dtype == np.float64 and recs.shape == (R, 3)
    # the sample's rows are the seeded choice of bench.sample_rows; two of them against the oracle on the bench's input
    sys.path.insert(0, ROOT)
    import bench
    idx = np.sort(np.random.default_rng(0xD0).choice(R, 256, replace=False))
    hop = bins - overlap
    iq = bench.synth_iq(torch, bins + hop * (R - 1), 0xC3, "cuda")
    bands = bench.make_bands(ro)
    for j in (0, 255):
        r = int(idx[j])
        want = oracle.stft(iq[r * hop:r * hop + bins].cpu().numpy(), bins, overlap)[0]
        assert np.abs(rows[j].astype(np.float64) - want).max() / want.max() <= 1e-5
        n, p, av = oracle.scan_rows(rows[j][None, :], bands.low_noise, bands.noise_width, bands.low_detect,
                                    bands.detect_width, bands.avg_bins)
        assert (n[0], p[0], av[0]) == tuple(recs[r]), r


@pytest.mark.parametrize("exchange,pattern", [("torch", "nccl"), ("capi", "nccl"), ("capi", "direct")])
def test_bench_c5_hash_is_the_hash_of_the_stream(ro, torch_cuda, exchange, pattern):
    torch = torch_cuda
    seconds = 900.0
    d = run_bench(["--full", "--workload", "c5", "--c5-seconds", str(seconds), "--exchange", exchange, "--pattern", pattern, "--steps", "2", "--warmup", "1",
                   "--prewarm", "1", "--no-cpu-baseline", "--no-strict", "--no-parity", "--no-streaming"])
    assert d["scaling"] == "strong"
    got = d["config"]["c5_hash_of_stitched_band_and_records"]
    # the same stream straight through the C ABI
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bench
    import util
    bins, overlap, fs = 32768, 24576, 48000
    total = int(seconds * fs)
    R = ro.row_count(total, bins, overlap)
    assert R == d["config"]["rows_per_step_per_gpu"]
    iq = util.c5_slice(torch, 0, (R - 1) * (bins - overlap) + bins, total_samples=total)
    lo = ro.frequency_to_bin(bins, fs, bench.JSON_SNAPSHOT[0])
    hi = ro.frequency_to_bin(bins, fs, bench.JSON_SNAPSHOT[1])
    rows = torch.empty((R, bins), dtype=torch.float32, device="cuda")
    tile = torch.empty((R, hi - lo), dtype=torch.float32, device="cuda")
    recs = torch.zeros((R, 3), dtype=torch.float32, device="cuda")
    with ro.Stft(bins=bins, overlap=overlap, bands=bench.make_bands(ro), tile=(lo, hi - lo)) as st:
        st.run_resident(iq, ro.RO_IQ_F32, iq.shape[0], 0, R, rows, d_tile=tile, d_records=recs,
                        stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    hh = hashlib.sha256()
    hh.update(tile.cpu().numpy().tobytes())
    hh.update(recs.cpu().numpy().tobytes())
    assert got == hh.hexdigest()[:32]
    assert np.array_equal(tile.cpu().numpy(), rows[:, lo:hi].cpu().numpy())
