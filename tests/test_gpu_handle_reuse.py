"""One long-lived handle against fresh handles, bit for bit: the paths that replace or regrow a handle's device blocks
(the band tables and their partial sums in both precisions, the four-step scratch), and create / run / destroy on every
kind of plan, which walks ro_stft_destroy over every group of buffers.

Nothing here asserts on free device memory: another tenant's allocations move the card's figure from moment to moment.
Overlaps are large, so that a handful of rows needs few samples beyond one row's."""
import numpy as np
import pytest

from util import noise_iq

pytestmark = pytest.mark.gpu

HOP = 512


def upload(torch, seed, bins, rows, hop=HOP):
    """(d_iq, samples) of sigma = 1 noise long enough for `rows` rows"""
    samples = (rows - 1) * hop + bins
    return torch.from_numpy(noise_iq(np.random.default_rng(seed), samples)).cuda(), samples


def band_on(ro, torch, st, d_iq, samples, first_col, cols, rows):
    d_band = torch.zeros((rows, cols), dtype=torch.float32, device="cuda")
    st.band_resident(d_iq, ro.RO_IQ_F32, samples, 0, rows, first_col, cols, d_band)
    torch.cuda.synchronize()
    return d_band


def check_band_reuse(ro, torch, bins, requests, **kw):
    d_iq, samples = upload(torch, bins, bins, max(r for _, _, r in requests))
    with ro.Stft(bins=bins, overlap=bins - HOP, **kw) as st:
        kept = [band_on(ro, torch, st, d_iq, samples, *req) for req in requests]
    for req, got in zip(requests, kept):
        with ro.Stft(bins=bins, overlap=bins - HOP, **kw) as st:
            want = band_on(ro, torch, st, d_iq, samples, *req)
        assert want.count_nonzero().item() == want.numel(), req
        assert torch.equal(got, want), req
    assert torch.equal(kept[0], kept[2][:kept[0].shape[0]])


def test_band_tables_replaced_and_partials_regrown_f32(ro, torch_cuda):
    """16384 bins, the smallest size band_plan takes: (100, 64 columns, 3 rows), then more columns and more rows (the
    tables change size, the partial sums grow), then the first band again (tables replaced, nothing regrown)"""
    check_band_reuse(ro, torch_cuda, 16384, [(100, 64, 3), (5000, 300, 9), (100, 64, 3)])


def test_band_tables_replaced_and_partials_regrown_f64(ro, torch_cuda):
    """the same on an RO_PRECISION_F64 handle of 131072 bins, the smallest its band kernels exist at"""
    check_band_reuse(ro, torch_cuda, 131072, [(100, 64, 2), (5000, 300, 5), (100, 64, 2)],
                     precision=ro.RO_PRECISION_F64)


def rows_on(ro, torch, st, d_iq, samples, rows):
    d_rows = torch.zeros((rows, st.bins), dtype=torch.float32, device="cuda")
    st.run_resident(d_iq, ro.RO_IQ_F32, samples, 0, rows, d_rows)
    torch.cuda.synchronize()
    return d_rows


def test_fourstep_scratch_regrown(ro, torch_cuda):
    """262144 bins: a launch of 1 row, of 3 (the block of Z between the two kernels grows), of 1 again"""
    torch = torch_cuda
    bins = 262144
    d_iq, samples = upload(torch, 4, bins, 3)
    with ro.Stft(bins=bins, overlap=bins - HOP) as st:
        kept = [rows_on(ro, torch, st, d_iq, samples, rows) for rows in (1, 3, 1)]
    for rows, got in zip((1, 3, 1), kept):
        with ro.Stft(bins=bins, overlap=bins - HOP) as st:
            want = rows_on(ro, torch, st, d_iq, samples, rows)
        assert want.count_nonzero().item() == want.numel(), rows
        assert torch.equal(got, want), rows
    assert torch.equal(kept[0], kept[1][:1]) and torch.equal(kept[0], kept[2])


PLANS = {
    "256": dict(bins=256),
    "32768_bands_tile_ln": dict(bins=32768, tile=(23278, 615), tile_ln=True),
    "65536_one_kernel": dict(bins=65536),
    "262144_fourstep": dict(bins=262144),
    "300_chirp_z": dict(bins=300),
    "4096_f64_registers": dict(bins=4096, f64=True),
    "131072_f64_scratch": dict(bins=131072, f64=True),
}


@pytest.mark.parametrize("plan", sorted(PLANS))
def test_create_run_destroy(ro, torch_cuda, plan):
    """three cycles of create, 2 rows, destroy: the third cycle's output equals the first's"""
    torch = torch_cuda
    kw = dict(PLANS[plan])
    bins, rows = kw.pop("bins"), 2
    hop = min(HOP, bins // 2)
    if kw.pop("f64", False):
        kw["precision"] = ro.RO_PRECISION_F64
    ln = kw.get("tile_ln", False)
    if ln:
        kw["bands"] = ro.Bands(low_noise=22000, noise_width=400, low_detect=23400, detect_width=300, avg_bins=27)
    d_iq, samples = upload(torch, 9, bins, rows, hop)
    cycles = []
    for _ in range(3):
        out = [torch.zeros((rows, bins), dtype=torch.float32, device="cuda")]
        with ro.Stft(overlap=bins - hop, bins=bins, **kw) as st:
            if ln:
                cols = kw["tile"][1]
                out += [torch.zeros((rows, cols), dtype=torch.float32, device="cuda") for _ in range(2)]
                out += [torch.zeros((rows, 2), dtype=torch.float32, device="cuda"),
                        torch.zeros((rows, 3), dtype=torch.float32, device="cuda")]
                st.run_resident_ln(d_iq, ro.RO_IQ_F32, samples, 0, rows, out[0], out[1], d_ln=out[2], d_minmax=out[3],
                                   d_records=out[4])
            else:
                st.run_resident(d_iq, ro.RO_IQ_F32, samples, 0, rows, out[0])
            torch.cuda.synchronize()
        cycles.append(out)
    assert cycles[0][0].count_nonzero().item() == rows * bins
    for a, b in zip(cycles[0], cycles[2]):
        assert a.any().item() and torch.equal(a, b)
