// ro_stft_capi.cpp -- the handle of the C ABI in include/ro_stft.h: create / destroy, the transform launches of every plan,
// the resident entry points (rows, spectra, scan, ln tile, timing), and scratch_for, the prelude of the plan-then-copy calls.
// Owns the window / twiddle tables in HBM.  The rest of the ABI: ro_abi_helpers.cpp, ro_exchange.cpp, ro_stream.cpp,
// ro_czt.cpp, and a file per plan-then-copy feature: ro_snapshots.cpp, ro_raw.cpp, ro_units.cpp, ro_periodic.cpp,
// ro_levels.cpp, ro_png.cpp, ro_png_deflate.cpp (ro_host.h lists who has what).
#include "ro_host.h"

using namespace ro::host;

namespace {

// per-stage twiddle tables in the layout apply_twiddles() reads:
//   stage with radix R after sub-transforms of length NS: entry (r-1)*NS + k = exp(-2 pi i r k / (NS R))
// evaluated in long double and rounded once to float.
std::vector<float2> build_twiddles(int bins)
{
    int radix[4];
    std::vector<float2> tw;
    if (!ro::stft_radices(bins, radix)) return tw;
    const long double two_pi = 8.0L * atanl(1.0L);
    long ns = radix[0];
    for (int s = 1; s < 4; ++s) {
        const int R = radix[s];
        if (R <= 1) continue;
        for (int r = 1; r < R; ++r)
            for (long k = 0; k < ns; ++k) {
                const long double ang = -two_pi * (long double)((long long)r * k) / (long double)(ns * R);
                tw.push_back(make_float2((float)cosl(ang), (float)sinl(ang)));
            }
        ns *= R;
    }
    return tw;
}

// exp(-2 pi i m / N) in double, correctly rounded from long double (strict-precision path)
std::vector<double2> build_full_twiddles_f64(int bins)
{
    std::vector<double2> tw((size_t)bins);
    const long double two_pi = 8.0L * atanl(1.0L);
    for (int m = 0; m < bins; ++m) {
        const long double ang = -two_pi * (long double)m / (long double)bins;
        tw[(size_t)m] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    return tw;
}

int validate_resident(const ro_stft *h, const void *d_iq, int format, int64_t samples,
                      int64_t first_row, int64_t rows, const float *d_rows, int64_t row_stride,
                      const float *d_tile, const ro_scan_record_t *d_records)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    if (format == RO_IQ_F64 && !h->f64reg)
        return fail(RO_ERR_UNSUPPORTED, "resident RO_IQ_F64 samples are taken by RO_PRECISION_F64 handles of 256 ... 65536 bins only");
    if (format != RO_IQ_F32 && format != RO_IQ_I16 && format != RO_IQ_F64)
        return fail(RO_ERR_INVALID, "resident input must be RO_IQ_F32, RO_IQ_I16 or RO_IQ_F64 (got %d)", format);
    if (rows < 0 || first_row < 0) return fail(RO_ERR_INVALID, "negative row range");
    if (rows == 0) return RO_OK;
    if (!d_iq) return fail(RO_ERR_INVALID, "null input pointer");
    if (!d_rows) return fail(RO_ERR_INVALID, "d_rows is required (the band tile is cut from the rows)");
    if (d_rows && row_stride < h->bins)
        return fail(RO_ERR_INVALID, "row_stride %lld < bins %d", (long long)row_stride, h->bins);
    if (d_tile && h->cfg.tile_cols <= 0) return fail(RO_ERR_INVALID, "tile output requested but tile_cols == 0");
    if (d_records && !h->cfg.enable_scan) return fail(RO_ERR_INVALID, "records requested but enable_scan == 0");
    if (d_records && !d_rows) return fail(RO_ERR_INVALID, "records need full rows (d_rows)");
    // every workgroup reads samples [r*hop, r*hop + bins): the last one must stay inside the buffer
    const int64_t last = (first_row + rows - 1) * (int64_t)h->hop + h->bins;
    if (last > samples)
        return fail(RO_ERR_INVALID, "rows [%lld,+%lld) need %lld samples, buffer holds %lld",
                    (long long)first_row, (long long)rows, (long long)last, (long long)samples);
    if (rows > (int64_t)0x0fffffff) return fail(RO_ERR_INVALID, "too many rows in one launch");
    return RO_OK;
}

ro::TileArgs make_tile_args(const ro_stft *h, const float *d_rows, int64_t row_stride, int64_t rows,
                            float *d_tile)
{
    ro::TileArgs t{};
    t.rows_in = d_rows;
    t.tile_out = d_tile;
    t.rows = rows;
    t.row_stride = row_stride;
    t.first = h->cfg.tile_first_col;
    t.cols = h->cfg.tile_cols;
    return t;
}

ro::ScanArgs make_scan_args(const ro_stft *h, const float *d_rows, int64_t row_stride, int64_t rows,
                            ro_scan_record_t *d_records)
{
    ro::ScanArgs s{};
    s.rows_in = d_rows;
    s.records = d_records;
    s.rows = rows;
    s.row_stride = row_stride;
    s.bins = h->bins;
    s.low_noise = h->cfg.bands.low_noise;
    s.noise_width = h->cfg.bands.noise_width;
    s.low_detect = h->cfg.bands.low_detect;
    s.detect_width = h->cfg.bands.detect_width;
    s.avg_bins = h->cfg.bands.avg_bins;
    return s;
}

ro::ScanSetsArgs make_scan_sets_args(const ro_stft *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                     ro_scan_record_t *d_extra)
{
    ro::ScanSetsArgs s{};
    s.rows_in = d_rows;
    s.extra = d_extra;
    s.rows = rows;
    s.row_stride = row_stride;
    s.bins = h->bins;
    s.count = h->extra_count;
    for (int i = 0; i < h->extra_count; ++i) s.sets[i] = h->extra[i];
    return s;
}

// scratch of the large sizes' scratch form (and of their complex spectra): rows per chunk and the blocks
int ensure_big_scratch(ro_stft *h)
{
    if (!h->spec_rows) {
        h->spec_rows = std::max<int64_t>(1, ((int64_t)RO_SPEC_SCRATCH_MB << 20) / ((int64_t)h->bins * 8));
        if (h->spec_rows > 65535) h->spec_rows = 65535;
    }
    if (!h->d_spec) HIP_TRY(h->d_spec.alloc((size_t)h->spec_rows * h->bins));
    if (!h->d_spec2) HIP_TRY(h->d_spec2.alloc((size_t)h->spec_rows * h->bins));
    return RO_OK;
}

// what every through-HBM FP64 launch of rows [first_row, +rows) is told (the pass loop adds ns / in / out per pass)
ro::BigArgsD make_bigd_args(const ro_stft *h, const void *d_iq, int64_t first_row, int64_t rows, float *d_rows,
                            int64_t row_stride)
{
    ro::BigArgsD b{};
    b.iq = d_iq;
    b.window = h->d_window;
    b.tw = h->d_tw_f64;
    b.first_row = first_row;
    b.rows = rows;
    b.row_stride = row_stride;
    b.hop = h->hop;
    b.n = h->bins;
    b.gain = h->cfg.iq_gain;
    b.rows_out = d_rows;
    return b;
}

#ifdef RO_DIAG
// Diagnostic builds only (RO_F64_FUSED=1): round 5's one-launch form of the through-HBM FP64 passes, the complex-double
// intermediate of a row handed between workgroups through the L2 of the XCD that makes it (ro_f64fused.hip; measured
// slower than the two launches, profiles/r05_f64_one_launch.txt; not in the product library).  The launch's give-up word
// travels to pinned host memory behind the kernel; a launch that gave up is reported by the NEXT call on the handle.
int launch_transform_f64_fused(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float *d_rows,
                               int64_t row_stride, hipStream_t s)
{
    if (h->h_f64_err && *h->h_f64_err != 0) {
        const unsigned code = *h->h_f64_err;
        *h->h_f64_err = 0;
        return fail(RO_ERR_HIP, "the previous RO_PRECISION_F64 launch gave up waiting for another workgroup (code %u: 1 = row "
                                "map, 2 = ring slot still being read, 3 = row's first half not complete); its rows are incomplete", code);
    }
    if (!h->f64_ring_rows) {
        int ring = RO_F64_RING_ROWS * 32768 / h->bins, wgs = RO_F64_WGS_PER_CU;
#ifdef RO_DIAG_KNOBS
        if (const char *e = getenv("RO_F64_RING_ROWS")) ring = atoi(e);
        if (const char *e = getenv("RO_F64_WGS")) wgs = atoi(e);
#endif
        h->f64_ring_rows = std::max(2, std::min(ring, ro::f64_fused_max_ring_rows()));
        h->f64_wgs_per_cu = std::max(1, std::min(wgs, 2));
    }
    // (each block on its own: a call after a failed one allocates what is missing and never launches without a block)
    if (!h->d_f64_ring) HIP_TRY(h->d_f64_ring.alloc((size_t)8 * h->f64_ring_rows * h->bins));
    if (!h->d_f64_ctl) HIP_TRY(h->d_f64_ctl.alloc(ro::f64_fused_ctl_bytes() / sizeof(unsigned)));
    if (!h->h_f64_err) {
        HIP_TRY(h->h_f64_err.alloc(1));
        *h->h_f64_err = 0;
    }
    const ro::BigArgsD b = make_bigd_args(h, d_iq, first_row, rows, d_rows, row_stride);
    HIP_TRY(ro::launch_f64_fused(format, b, h->d_f64_ring, h->d_f64_ctl, h->f64_ring_rows, h->f64_wgs_per_cu, s));
    HIP_TRY(hipMemcpyAsync(h->h_f64_err, h->d_f64_ctl + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    return RO_OK;
}
#endif

// the register kernel's arguments (ro_f64reg.hip); out: magnitude rows, or complex spectra with r.spectra = 1
ro::F64RegArgs make_f64reg_args(const ro_stft *h, const void *d_iq, int64_t first_row, int64_t rows, float *out, int64_t stride)
{
    ro::F64RegArgs r{};
    r.iq = d_iq;
    r.window_k = h->d_f64r_window;
    r.tw0 = h->d_f64r_tw[0];
    r.tw1 = h->d_f64r_tw[1];
    r.tw2 = h->d_f64r_tw[2];
    r.tw3 = h->d_f64r_tw[3];
    r.rows_out = out;
    r.first_row = first_row;
    r.rows = rows;
    r.row_stride = stride;
    r.hop = h->hop;
    r.gain = h->cfg.iq_gain;
    return r;
}

// RO_PRECISION_F64: every size as radix-16 passes in double through HBM scratch, in chunks that fit it
int launch_transform_f64(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float *d_rows,
                         int64_t row_stride, hipStream_t s)
{
#ifdef RO_DIAG
    if (const char *e = getenv("RO_F64_FUSED"))
        if (atoi(e) != 0 && ro::f64_fused_supported(h->bins))
            return launch_transform_f64_fused(h, d_iq, format, first_row, rows, d_rows, row_stride, s);
#endif
    if (h->f64reg) {
        ro::F64RegArgs r = make_f64reg_args(h, d_iq, first_row, rows, d_rows, row_stride);
        r.stamps = h->d_stamps;
        HIP_TRY(ro::launch_f64reg(h->bins, format, r, s));
        return RO_OK;
    }
    if (!h->scratch_rows_d) {
        int64_t mib = RO_F64_SCRATCH_MB;
#ifdef RO_DIAG
        if (const char *e = getenv("RO_F64_SCRATCH_MB")) mib = std::max(1, atoi(e));     // tools/r4/strict_sweep.sh
#endif
        h->scratch_rows_d = std::max<int64_t>(1, (mib << 20) / ((int64_t)h->bins * 16));
    }
    for (auto &blk : h->d_scratch_d)             // (each block on its own: a call after a failed one never launches without one)
        if (!blk) HIP_TRY(blk.alloc((size_t)h->scratch_rows_d * h->bins));
    int radix[8];
    const int passes = ro::f64_radices(h->bins, radix);
    if (passes < 2) return fail(RO_ERR_UNSUPPORTED, "no FP64 pass plan for bins = %d", h->bins);
    for (int64_t done = 0; done < rows; done += h->scratch_rows_d) {
        const int64_t n = std::min(h->scratch_rows_d, rows - done);
        ro::BigArgsD b = make_bigd_args(h, d_iq, first_row + done, n, d_rows + done * row_stride, row_stride);
        // two passes per kernel where the pair fits its LDS tile (radix 16 followed by any radix, bins >= 4096): half
        // the trips through the scratch blocks
        int ns = 1, hop_idx = 0;
        for (int p = 0; p < passes;) {
            const bool pair = h->bins >= 4096 && p + 1 < passes && radix[p] == 16;
            const int last_p = pair ? p + 1 : p;
            b.ns = ns;
            b.in = h->d_scratch_d[(hop_idx + 1) & 1];
            b.out = h->d_scratch_d[hop_idx & 1];
            if (pair) HIP_TRY(ro::launch_f64_pair(radix[p + 1], p == 0, last_p == passes - 1, format, b, s));
            else HIP_TRY(ro::launch_f64_pass(radix[p], p == 0, p == passes - 1, format, b, s));
            for (int q = p; q <= last_p; ++q) ns *= radix[q];
            p = last_p + 1;
            ++hop_idx;
        }
    }
    return RO_OK;
}

}  // namespace

namespace ro {
namespace host {

int check_bands(const ro_stft *h, const ro_bands_t &b)
{
    if (b.noise_width <= 0 || b.detect_width <= 0 || b.avg_bins <= 0)
        return fail(RO_ERR_INVALID, "bands: widths and avg_bins must be positive");
    if (b.low_noise < 0 || b.low_noise + b.noise_width > h->bins)
        return fail(RO_ERR_INVALID, "bands: noise band [%d,+%d) outside [0,%d)", b.low_noise,
                    b.noise_width, h->bins);
    if (b.low_detect < 0 || b.low_detect + b.detect_width > h->bins)
        return fail(RO_ERR_INVALID, "bands: detect band [%d,+%d) outside [0,%d)", b.low_detect,
                    b.detect_width, h->bins);
    return RO_OK;
}

ro::StftArgs make_stft_args(const ro_stft *h, const void *d_iq, int64_t first_row, int64_t rows,
                            float *d_rows, int64_t row_stride, float *d_tile,
                            ro_scan_record_t *d_records, float *d_ln)
{
    ro::StftArgs a{};
    a.iq = d_iq;
    a.window = h->d_window;
    a.window_k = h->d_window_k;
    a.window_k32 = h->d_window_k32;
    a.twiddles = h->d_twiddles;
    a.twiddles_k = h->d_twiddles_k;
    a.rows_out = d_rows;
    a.first_row = first_row;
    a.rows = rows;
    a.row_stride = row_stride;
    a.hop = h->hop;
    a.gain = (float)h->cfg.iq_gain;
    a.stamps = h->d_stamps;
    a.spare_cus = h->cfg.spare_cus_per_xcd;
    // plans with a fused epilogue scan / tile take them here; for the others the caller launches the separate kernels
    if (!h->f64 && ro::stft_fuses_scan(h->bins)) {
        a.records = d_records;
        a.low_noise = h->cfg.bands.low_noise;
        a.noise_width = h->cfg.bands.noise_width;
        a.low_detect = h->cfg.bands.low_detect;
        a.detect_width = h->cfg.bands.detect_width;
        a.avg_bins = h->cfg.bands.avg_bins;
        a.tile_out = d_tile;
        a.tile_first = h->cfg.tile_first_col;
        a.tile_cols = h->cfg.tile_cols;
        a.ln_out = d_tile ? d_ln : nullptr;
        a.ln_part = h->d_ln_part;
    }
    return a;
}

// d_ln / d_minmax: the tile's log and the rows' min / max of it (tile_ln); need d_tile
int launch_tile_and_scan(ro_stft *h, const float *d_rows, int64_t row_stride, int64_t rows, float *d_tile,
                         ro_scan_record_t *d_records, hipStream_t s, float *d_ln, float *d_minmax, ro_scan_record_t *d_extra,
                         const ro::CutArgs *cut)
{
    const bool want_ln = d_tile && (d_ln || d_minmax);
    if (!h->f64 && ro::stft_fuses_scan(h->bins)) {                  // tile, log and records written by the transform
        if (want_ln && d_minmax) HIP_TRY(ro::launch_ln_finish(h->d_ln_part, d_minmax, rows, s));
    } else {
        if (d_tile) HIP_TRY(ro::launch_tile(make_tile_args(h, d_rows, row_stride, rows, d_tile), s));
        if (want_ln) HIP_TRY(ro::launch_ln_rows(d_tile, d_ln, d_minmax, rows, h->cfg.tile_cols, s));
        if (d_records) HIP_TRY(ro::launch_scan(make_scan_args(h, d_rows, row_stride, rows, d_records), s));
    }
    // the extra band sets, from the rows in HBM whatever wrote the primary's record (the fused epilogue is frozen)
    if (d_extra && h->extra_count > 0)
        HIP_TRY(ro::launch_scan_sets(make_scan_sets_args(h, d_rows, row_stride, rows, d_extra), s));
    // the tile windows, a plain copy out of the rows in HBM for every plan alike (no transform's epilogue knows them)
    if (cut) {
        ro::CutArgs c = *cut;
        c.rows_in = d_rows;
        c.rows = rows;
        c.row_stride = row_stride;
        HIP_TRY(ro::launch_cut_windows(c, s));
    }
    return RO_OK;
}

// scratch of the fused log: the two tile waves' partial min / max, 4 floats per row of the launch
int ensure_ln_part(ro_stft *h, int64_t rows)
{
    if (rows <= h->ln_part_rows) return RO_OK;
    // sized generously the first time (16 bytes per row) and doubled after that, so that the device-wide wait a
    // regrow needs -- an earlier launch may still be writing the old block -- happens at most a few times per handle
    int64_t want = std::max<int64_t>(rows, std::max<int64_t>(65536, 2 * h->ln_part_rows));
    if (h->d_ln_part) (void)hipDeviceSynchronize();
    h->ln_part_rows = 0;
    HIP_TRY(h->d_ln_part.alloc((size_t)want * 4));
    h->ln_part_rows = want;
    return RO_OK;
}

int grow_scratch(DeviceBlock<char> &block, size_t need)
{
    if (block.count() >= need) return RO_OK;
    if (block) HIP_TRY(hipDeviceSynchronize());                   // (an earlier launch may still be using the old block)
    HIP_TRY(block.alloc(need));
    return RO_OK;
}

int device_cus(ro_stft *h, int *cus)
{
    if (h->cus == 0) HIP_TRY(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device));
    *cus = h->cus;
    return RO_OK;
}

int scratch_for(ro_stft *h, DeviceBlock<char> &block, size_t need, int *cus)
{
    HIP_TRY(hipSetDevice(h->device));
    const int rc = device_cus(h, cus);
    return rc != RO_OK ? rc : grow_scratch(block, need);
}

// complex spectra of rows [first_row, +rows) of a large size (bins = dec x 32768), bin k at element k of each row:
// fold_kernel, the N = 32768 kernel in spectra mode on its rows, interleave2_kernel
int launch_spectra_big(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float2 *d_out,
                       int64_t out_stride, hipStream_t s)
{
    int rc = ensure_big_scratch(h);
    if (rc != RO_OK) return rc;
    for (int64_t done = 0; done < rows; done += h->spec_rows) {
        const int64_t n = std::min(h->spec_rows, rows - done);
        ro::FoldArgs f{};
        f.iq = d_iq;
        f.window = h->d_window;
        f.rot = h->d_tw_combine;
        f.out = h->d_spec;
        f.first_row = first_row + done;
        f.rows = n;
        f.hop = h->hop;
        f.m = h->sub_bins;
        f.dec = h->dec;
        f.gain = (float)h->cfg.iq_gain;
        HIP_TRY(ro::launch_fold(format, f, s));
        ro::StftArgs a = make_stft_args(h, h->d_spec, 0, n * h->dec, nullptr, 0);
        a.window = h->d_ones;
        a.window_k = h->d_ones;
        a.window_k32 = h->d_ones;
        a.hop = h->sub_bins;
        a.gain = 0.0f;
        a.spec_out = h->d_spec2;
        a.spec_stride = h->sub_bins;
        HIP_TRY(ro::launch_stft(h->sub_bins, RO_FMT_F32, a, s));
        ro::Interleave2Args t{};
        t.in = h->d_spec2;
        t.out = d_out + done * out_stride;
        t.rows = n;
        t.out_stride = out_stride;
        t.m = h->sub_bins;
        t.dec = h->dec;
        HIP_TRY(ro::launch_interleave2(t, s));
    }
    return RO_OK;
}

int launch_transform(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float *d_rows,
                     int64_t row_stride, hipStream_t s, float *d_tile, ro_scan_record_t *d_records, float *d_ln)
{
    if (h->f64) return launch_transform_f64(h, d_iq, format, first_row, rows, d_rows, row_stride, s);
    if (h->czt) return launch_transform_czt(h, d_iq, format, first_row, rows, d_rows, row_stride, s);
    if (!h->big) {
        if (d_tile && d_ln && ro::stft_fuses_scan(h->bins)) {
            int rc = ensure_ln_part(h, rows);
            if (rc != RO_OK) return rc;
        }
        ro::StftArgs a = make_stft_args(h, d_iq, first_row, rows, d_rows, row_stride, d_tile, d_records, d_ln);
        HIP_TRY(ro::launch_stft(h->bins, format, a, s));
        return RO_OK;
    }
    if (h->four) {
        {
            int64_t mib = RO_FOUR_SCRATCH_MB;
#ifdef RO_DIAG_KNOBS
            if (const char *e = getenv("RO_FOUR_SCRATCH_MB")) mib = std::max<int64_t>(4, atoll(e));
#endif
            const int64_t limit = std::max<int64_t>(1, (mib << 20) / ((int64_t)h->bins * 8));
            const int64_t want = std::min(limit, rows);
            if (want > h->four_rows) {
                // The old block may still be in use: by launches queued on the caller's stream, on the handle's own, or on
                // a streaming slot's (captured graphs are not taken for these sizes, run_stream_batch, but a handle may be
                // used both ways).  Everything the handle has queued anywhere is waited for before the block goes.
                if (h->d_four_z) {
                    HIP_TRY(hipStreamSynchronize(s));
                    if (h->stream && h->stream != s) HIP_TRY(hipStreamSynchronize(h->stream));
                    for (ro_stft::Slot &sl : h->slot)
                        if (sl.gstream && sl.gstream != s) HIP_TRY(hipStreamSynchronize(sl.gstream));
                }
                h->four_rows = 0;
                HIP_TRY(h->d_four_z.alloc((size_t)want * h->bins * 2));
                h->four_rows = want;
            }
        }
        for (int64_t done = 0; done < rows; done += h->four_rows) {
            ro::FourArgs f{};
            f.iq = d_iq;
            f.first_row = first_row + done;
            f.rows = std::min(h->four_rows, rows - done);
            f.hop = h->hop;
            f.gain = (float)h->cfg.iq_gain;
            f.n1 = h->bins / 1024;
            f.window_a = h->d_four_window;
            f.tw_a = h->d_four_tw_a;
            f.tw_b = h->d_four_tw_b;
            f.tw_r = h->d_four_tw_r;
            f.z = h->d_four_z;
            f.rows_out = d_rows + done * row_stride;
            f.row_stride = row_stride;
            f.spare_cus = h->cfg.spare_cus_per_xcd;
            HIP_TRY(ro::launch_fourstep(format, f, s));
        }
        return RO_OK;
    }
    if (h->dec > 1 && h->dif) {
        // one kernel, no scratch: kernel row srow * dec + q makes the bins q + dec k' of stream row srow
        int log2 = 0;
        while ((1 << log2) < h->dec) ++log2;
        ro::StftArgs a = make_stft_args(h, d_iq, first_row, rows * h->dec, d_rows, row_stride);
        a.window = h->d_window;
        a.window_k = h->d_window_dif;
        a.dec = h->dec;
        a.dec_log2 = log2;
        a.dif_tw = h->d_dif_tw;
        a.dif_shift = h->d_dif_shift;
        a.big_form = 1;
        HIP_TRY(ro::launch_stft(h->sub_bins, format, a, s));
        return RO_OK;
    }
    return fail(RO_ERR_STATE, "internal: no transform plan for bins = %d", h->bins);
}

}  // namespace host
}  // namespace ro

extern "C" int ro_bins_supported(int bins)
{
    return (ro::stft_supported(bins) || ro::big_supported(bins) || czt_length(bins) > 0) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------
extern "C" int ro_stft_create(const ro_stft_config_t *cfg_in, ro_stft_t **out)
{
    if (!cfg_in || !out) return fail(RO_ERR_INVALID, "ro_stft_create: null argument");
    *out = nullptr;
    const ro_stft_config_t *cfg = cfg_in;          // re-pointed at a full-size copy once struct_size is known
    // ABI growth: fields are only ever appended; a caller built against ABI 1 passes the shorter struct and gets the
    // defaults (0) for what it does not know
    const size_t abi1_size = offsetof(ro_stft_config_t, precision);
    if (cfg->struct_size != sizeof(ro_stft_config_t) && cfg->struct_size != abi1_size)
        return fail(RO_ERR_INVALID, "ro_stft_create: struct_size %u is neither %zu (ABI 2) nor %zu (ABI 1)",
                    cfg->struct_size, sizeof(ro_stft_config_t), abi1_size);
    ro_stft_config_t cfg_full{};
    std::memcpy(&cfg_full, cfg_in, cfg_in->struct_size);
    cfg_full.struct_size = sizeof(ro_stft_config_t);
    cfg = &cfg_full;
    if (cfg->precision == 2)                       // ABI 4's RO_PRECISION_F64_ONE_LAUNCH: an experiment, retired from the library
        return fail(RO_ERR_UNSUPPORTED, "precision 2 (the one-launch form of RO_PRECISION_F64) is no longer part of the library: "
                                        "use RO_PRECISION_F64");
    if (cfg->precision != RO_PRECISION_F32 && cfg->precision != RO_PRECISION_F64)
        return fail(RO_ERR_INVALID, "unknown precision %d", cfg->precision);
    if (cfg->tile_ln != 0 && cfg->tile_ln != 1) return fail(RO_ERR_INVALID, "tile_ln must be 0 or 1");
    if (cfg->tile_ln && cfg->tile_cols <= 0) return fail(RO_ERR_INVALID, "tile_ln needs a tile (tile_cols > 0)");
    if (!ro_bins_supported(cfg->bins))
        return fail(RO_ERR_UNSUPPORTED, "bins = %d has no kernel (powers of two 256..1048576, other even lengths "
                                        "258..524286)", cfg->bins);
    if (czt_length(cfg->bins) && cfg->precision != RO_PRECISION_F32)
        return fail(RO_ERR_UNSUPPORTED, "RO_PRECISION_F64 is available for power-of-two bins only");
    if (cfg->iq_phase_shift != 0)
        return fail(RO_ERR_UNSUPPORTED, "iq_phase_shift != 0 is undefined behaviour in the reference "
                                        "(src/FFTBackend.cpp:67-71) and is not supported");
    if (cfg->sample_rate <= 0) return fail(RO_ERR_INVALID, "sample_rate must be positive");
    if (cfg->spare_cus_per_xcd < 0 || cfg->spare_cus_per_xcd > 16)
        return fail(RO_ERR_INVALID, "spare_cus_per_xcd must be in [0, 16]");
    if (cfg->window_kind == RO_WINDOW_CUSTOM && !cfg->window_table)
        return fail(RO_ERR_INVALID, "RO_WINDOW_CUSTOM needs window_table");
    if (cfg->window_kind < RO_WINDOW_NUTTALL || cfg->window_kind > RO_WINDOW_CUSTOM)
        return fail(RO_ERR_INVALID, "unknown window_kind %d", cfg->window_kind);
    if (cfg->tile_cols < 0 || cfg->tile_first_col < 0 || cfg->tile_first_col + cfg->tile_cols > cfg->bins)
        return fail(RO_ERR_INVALID, "tile [%d,+%d) outside [0,%d)", cfg->tile_first_col, cfg->tile_cols,
                    cfg->bins);

    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(RO_ERR_HIP, "device %d not present (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));

    ro_stft *h = new (std::nothrow) ro_stft();
    if (!h) return fail(RO_ERR_NOMEM, "out of host memory");
    h->cfg = *cfg;
    h->cfg.window_table = nullptr;
    h->bins = cfg->bins;
    h->overlap = ro_clamp_overlap(cfg->bins, cfg->overlap);
    h->hop = h->bins - h->overlap;
    h->device = cfg->device;
    if (cfg->enable_scan) {
        int rc = check_bands(h, cfg->bands);
        if (rc != RO_OK) { delete h; return rc; }
    }

    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, cfg->device);
    if (e != hipSuccess) { delete h; return fail(RO_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(e)); }
    h->device_name = prop.name;
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        delete h;
        return fail(RO_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 only",
                    cfg->device, prop.gcnArchName);
    }
    // The N = 32768 kernel (and what is built on it) wants 132 KiB of LDS for ONE workgroup and spreads its grid over
    // eight XCDs (blockIdx % 8, round-robin dispatch): say so here rather than with an opaque launch error later.  A
    // partition mode with fewer XCDs per device only loses the placement (rows of one XCD's run no longer share an L2).
    if ((prop.maxSharedMemoryPerMultiProcessor > 0 && (size_t)prop.maxSharedMemoryPerMultiProcessor < (size_t)132 * 1024) ||
        prop.multiProcessorCount < 8) {
        const size_t lds = (size_t)prop.maxSharedMemoryPerMultiProcessor;
        const int cus = prop.multiProcessorCount;
        delete h;
        return fail(RO_ERR_UNSUPPORTED, "device %d offers %zu bytes of LDS per CU and %d CUs; the kernels need 135168 for one workgroup and 8",
                    cfg->device, lds, cus);
    }

    // ... and the persistent kernels hand rows out in eight runs, one per XCD (blockIdx % 8 under round-robin dispatch;
    // ro_stft32k.hip, ro_kernels.hip, ro_fourstep.hip, ro_f64reg.hip).  A partition mode with another number of XCDs
    // computes the same rows and only loses the placement (rows of one run no longer share an L2): said once, not refused.
    {
        int xccs = 0;
        if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, cfg->device) == hipSuccess) {
            static bool said = false;
            if (xccs > 0 && xccs != 8 && !said) {            // (0: a runtime that answers without knowing)
                said = true;
                fprintf(stderr, "libro_stft: device %d reports %d XCDs; the kernels' row placement is laid out for 8 (an MI355X in "
                                "SPX mode): rows are unaffected, the L2 sharing between neighbouring rows is lost\n", cfg->device, xccs);
            }
        } else {
            (void)hipGetLastError();
        }
    }

    h->window.resize(h->bins);
    if (cfg->window_kind == RO_WINDOW_CUSTOM)
        std::memcpy(h->window.data(), cfg->window_table, sizeof(float) * h->bins);
    else
        build_window(cfg->window_kind, h->bins, h->window.data());
    h->big = ro::big_supported(h->bins);
    h->f64 = cfg->precision != RO_PRECISION_F32;
    h->czt_m = czt_length(h->bins);
    h->czt = h->czt_m > 0;
    if (h->big && !h->f64) {
        // bins = dec x 32768, decimation in frequency on the largest single-pass plan:
        //   X[q + dec k'] = sum_m W_N^(m k') { W_bins^(m q) sum_r W_dec^(r q) w[m + N r] x[m + N r] }
        // 65536, 131072: ONE kernel (ro::stft_kernel MODE 3) that sums the row's dec blocks itself -- dec x the row
        // through L2 per output row, nothing extra through HBM (0.27 / 0.19 of the HBM peak; it was 0.11 / 0.06 at
        // 262144 / 524288, where its 4-byte stores `dec` floats apart cost an L2 write request each).
        // 262144 ... 1048576: the four-step pair of kernels (ro_fourstep.hip) for the magnitude rows.
        // Complex spectra of every large size: fold_kernel writes the braces to scratch, the N = 32768 kernel transforms
        // those rows, interleave2_kernel puts the bins in place (launch_spectra_big).  Rounds 2 and 3 made the magnitude
        // rows of dec >= 8 that way too (0.10-0.13 of the peak; profiles/r04_fourstep.txt has the A/B).
        // (Diagnostic builds: RO_BIG_FORM=dif forces the one-kernel form.)
        const int sub = 32768, dec = h->bins / sub;
        bool four = ro::fourstep_supported(h->bins);
#ifdef RO_DIAG_KNOBS
        if (const char *e = getenv("RO_BIG_FORM")) four = std::strcmp(e, "dif") != 0 && four;
#endif
        h->four = four;
        h->dif = !four;
        h->sub_bins = sub;
        h->dec = dec;
    }
    const int plan_bins = h->czt ? 0 : h->big ? h->sub_bins : h->bins;   // whose stage tables this handle needs (0: none)
    std::vector<float2> tw = plan_bins ? build_twiddles(plan_bins) : std::vector<float2>();
    if (plan_bins && (int)tw.size() != ro::stft_twiddle_count(plan_bins)) {
        delete h;
        return fail(RO_ERR_STATE, "internal: twiddle table size mismatch");
    }

#define CREATE_TRY(expr)                                                                   \
    do {                                                                                   \
        hipError_t e2_ = (expr);                                                           \
        if (e2_ != hipSuccess) {                                                           \
            int rc2_ = fail(RO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e2_));   \
            ro_stft_destroy(h);                                                            \
            return rc2_;                                                                   \
        }                                                                                  \
    } while (0)
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CREATE_TRY(hipEventCreate(&h->ev0));
    CREATE_TRY(hipEventCreate(&h->ev1));
    CREATE_TRY(h->d_window.upload(h->window));
    CREATE_TRY(h->d_ln_keys.alloc(16 * 2));                      // (never memset: every call initialises the pair it uses)
    if (tw.empty()) CREATE_TRY(h->d_twiddles.alloc(1));          // (a handle without stage tables still hands a pointer on)
    else CREATE_TRY(h->d_twiddles.upload(tw));
    if (!h->big && !h->czt) {
        std::vector<float> wk((size_t)h->bins);
        if (!ro::stft_window_layout(h->bins, h->window.data(), wk.data())) {
            ro_stft_destroy(h);
            return fail(RO_ERR_UNSUPPORTED, "no window layout for bins=%d", h->bins);
        }
        CREATE_TRY(h->d_window_k.upload(wk));
        if (h->bins == 32768) {
            ro::stft32k_window_layout(h->window.data(), wk.data());
            CREATE_TRY(h->d_window_k32.upload(wk));
        }
    }
    if (plan_bins) {
        const int units = ro::stft_packed_twiddle_count(plan_bins);
        std::vector<float4> pk((size_t)std::max(units, 1));
        if (units > 0) ro::stft_pack_twiddles(plan_bins, tw.data(), pk.data());
        CREATE_TRY(h->d_twiddles_k.upload(pk));
    }
    if (h->f64) {
        std::vector<double2> full = build_full_twiddles_f64(h->bins);
        CREATE_TRY(h->d_tw_f64.upload(full));
        h->f64reg = ro::f64reg_supported(h->bins);
#ifdef RO_DIAG
        if (const char *e = getenv("RO_F64_HBM")) h->f64reg = h->f64reg && atoi(e) == 0;   // the through-HBM passes, for A/B
#endif
        if (h->f64reg) {
            ro::F64RegTables t;
            ro::f64reg_tables(h->bins, h->window.data(), t);
            CREATE_TRY(h->d_f64r_window.upload(t.window_k));
            const std::vector<double2> *tabs[4] = {&t.tw0, &t.tw1, &t.tw2, &t.tw3};
            for (int i = 0; i < 4; ++i)
                if (!tabs[i]->empty()) CREATE_TRY(h->d_f64r_tw[i].upload(*tabs[i]));
        }
    }
    if (h->big && h->dec > 1) {
        // the rotations W_bins^(q m), [dec][sub_bins], each rounded once from long double
        std::vector<float2> tc((size_t)h->bins);
        const long double two_pi = 8.0L * atanl(1.0L);
        for (int r = 0; r < h->dec; ++r)
            for (int k = 0; k < h->sub_bins; ++k) {
                const long double ang = -two_pi * (long double)((long long)r * k) / (long double)h->bins;
                tc[(size_t)r * h->sub_bins + k] = make_float2((float)cosl(ang), (float)sinl(ang));
            }
        CREATE_TRY(h->d_tw_combine.upload(tc));
    }
    if (h->big && h->dec > 1) {
        std::vector<float> ones((size_t)h->sub_bins, 1.0f);
        CREATE_TRY(h->d_ones.upload(ones));
    }
    if (h->dif) {
        std::vector<float> wk((size_t)h->bins);
        for (int r = 0; r < h->dec; ++r)
            if (!ro::stft_window_layout(h->sub_bins, h->window.data() + (size_t)r * h->sub_bins,
                                        wk.data() + (size_t)r * h->sub_bins)) {
                ro_stft_destroy(h);
                return fail(RO_ERR_UNSUPPORTED, "no window layout for bins=%d", h->sub_bins);
            }
        CREATE_TRY(h->d_window_dif.upload(wk));
        std::vector<float2> td((size_t)h->dec);
        const long double two_pi = 8.0L * atanl(1.0L);
        for (int j = 0; j < h->dec; ++j) {
            // (quarter turns exact: cosl(pi/2) is 6e-20, not 0)
            const long double ang = -two_pi * (long double)j / (long double)h->dec;
            long double c = cosl(ang), sn = sinl(ang);
            if ((4 * j) % h->dec == 0) { c = roundl(c); sn = roundl(sn); }
            td[(size_t)j] = make_float2((float)c, (float)sn);
        }
        CREATE_TRY(h->d_dif_tw.upload(td));
        // residue q's rotation W_bins^(m q) as a shift of the bin index by q / dec: per stage (32, 32 x 32, 32^3 points
        // behind it) the powers 1, 2, 4, 8, 16 of exp(-2 pi i (q / dec) / M), each rounded once from long double
        std::vector<float2> ts((size_t)h->dec * 16, make_float2(1.0f, 0.0f));
        const long double span[3] = {32.0L, 1024.0L, 32768.0L};
        for (int q = 0; q < h->dec; ++q)
            for (int st = 0; st < 3; ++st)
                for (int i = 0; i < 5; ++i) {
                    const long double ang = -two_pi * ((long double)q / (long double)h->dec) * (long double)(1 << i) / span[st];
                    ts[(size_t)q * 16 + st * 5 + i] = make_float2((float)cosl(ang), (float)sinl(ang));
                }
        CREATE_TRY(h->d_dif_shift.upload(ts));
    }
    if (h->four) {
        std::vector<float> wa;
        std::vector<float2> ta, tb, tr;
        ro::fourstep_tables(h->bins, h->window.data(), wa, ta, tb, tr);
        CREATE_TRY(h->d_four_window.upload(wa));
        CREATE_TRY(h->d_four_tw_a.upload(ta));
        CREATE_TRY(h->d_four_tw_b.upload(tb));
        CREATE_TRY(h->d_four_tw_r.upload(tr));
    }
    if (h->czt) {
        const int rc = czt_setup(h);
        if (rc != RO_OK) { ro_stft_destroy(h); return rc; }
    }
#undef CREATE_TRY

    // what travels to the host in the streaming path: the tile when one is configured, else whole rows
    h->out_first = cfg->tile_cols > 0 ? cfg->tile_first_col : 0;
    h->out_cols = cfg->tile_cols > 0 ? cfg->tile_cols : h->bins;
    // streaming buffers are allocated lazily by the first push
    h->batch_rows = cfg->max_batch_rows > 0 ? cfg->max_batch_rows
                                            : std::max(1, (64 << 20) / (h->bins * 4));   // ~64 MiB of rows
#ifdef RO_DIAG_KNOBS
    if (const char *e = getenv("RO_GRAPH_TIME_EVERY")) h->diag_time_every = atoi(e);       // tools/r5/host_calls_ab.py
    if (const char *e = getenv("RO_GRAPH_TWO_EVENTS")) h->diag_done_only = atoi(e) == 0;
    if (const char *e = getenv("RO_GRAPH_DIRECT")) h->diag_direct = atoi(e);
#endif
    *out = h;
    return RO_OK;
}

extern "C" int ro_stft_destroy(ro_stft_t *h)
{
    if (!h) return RO_OK;
    (void)hipSetDevice(h->device);
    if (h->s_in) (void)hipStreamSynchronize(h->s_in);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->s_out) (void)hipStreamSynchronize(h->s_out);
    for (ro_stft::Slot &sl : h->slot)                       // graphed batches and their downloads run on the slots' own streams
        if (sl.gstream) (void)hipStreamSynchronize(sl.gstream);
    free_stream_slots(h);
    while (!h->ready.empty()) {
        destroy_batch(h->ready.front());
        h->ready.pop_front();
    }
    for (Batch *b : h->batch_pool) destroy_batch(b);
    if (h->inner) (void)ro_stft_destroy(h->inner);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;                                       // ... and with it every device and pinned block (ro_owned.h)
    return RO_OK;
}

#ifdef RO_DIAG
// Diagnostic builds only (-DRO_DIAG=1; not in include/ro_stft.h, not in the product library): allocate / read the per-wave
// phase stamps that a -DRO_STAMPS=1 / -DRO_STAMPS32K=1 / -DRO_F64R_STAMPS=1 build of the kernels fills.
extern "C" int ro_stft_debug_stamps(ro_stft_t *h, unsigned long long *out, int max_words)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    const int words = 4096 * 16;
    if (!h->d_stamps) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->d_stamps.alloc(words));
        HIP_TRY(hipMemset(h->d_stamps, 0, sizeof(unsigned long long) * words));
        return RO_OK;
    }
    if (out) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(out, h->d_stamps, sizeof(unsigned long long) * std::min(words, max_words),
                          hipMemcpyDeviceToHost));
    }
    return RO_OK;
}
#endif

extern "C" int ro_stft_get_window(const ro_stft_t *h, float *out)
{
    if (!h || !out) return fail(RO_ERR_INVALID, "null argument");
    std::memcpy(out, h->window.data(), sizeof(float) * h->bins);
    return RO_OK;
}

extern "C" int ro_stft_hop(const ro_stft_t *h) { return h ? h->hop : fail(RO_ERR_INVALID, "null handle"); }
extern "C" int ro_stft_bins(const ro_stft_t *h) { return h ? h->bins : fail(RO_ERR_INVALID, "null handle"); }

extern "C" int ro_stft_device_name(const ro_stft_t *h, char *buf, size_t len)
{
    if (!h || !buf || len == 0) return fail(RO_ERR_INVALID, "null argument");
    std::snprintf(buf, len, "%s", h->device_name.c_str());
    return RO_OK;
}

extern "C" int ro_stft_set_bands(ro_stft_t *h, const ro_bands_t *bands)
{
    if (!h || !bands) return fail(RO_ERR_INVALID, "null argument");
    int rc = check_bands(h, *bands);
    if (rc != RO_OK) return rc;
    h->cfg.bands = *bands;
    h->cfg.enable_scan = 1;
    return RO_OK;
}

// ---------------------------------------------------------------------------
// resident path
// ---------------------------------------------------------------------------
// ro_stft_run_resident, ro_stft_run_resident_sets and ro_stft_run_resident_ln: the same launches, plus scan_sets_kernel
// when d_extra is given, plus the tile's log and its range when d_ln / d_minmax are
static int run_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row, int64_t rows,
                        float *d_rows, int64_t row_stride, float *d_tile, ro_scan_record_t *d_records,
                        ro_scan_record_t *d_extra, void *stream, float *d_ln = nullptr, float *d_minmax = nullptr,
                        const ro::CutArgs *cut = nullptr)
{
    int rc = validate_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile,
                               d_records);
    if (rc != RO_OK) return rc;
    if (d_extra && h->extra_count == 0)
        return fail(RO_ERR_STATE, "extra records requested but no extra band sets are set (ro_stft_set_extra_bands)");
    if (rows == 0) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;      // NULL = the default (null) stream, like any HIP launch
    // (the fused epilogue always writes the log when asked for its range: the partial min / max come with it)
    rc = launch_transform(h, d_iq, format, first_row, rows, d_rows, row_stride, s, d_tile, d_records, d_ln);
    if (rc != RO_OK) return rc;
    rc = launch_tile_and_scan(h, d_rows, row_stride, rows, d_tile, d_records, s, d_ln, d_minmax, d_extra, cut);
    if (rc != RO_OK) return rc;
    h->stat_launches += 1;
    h->stat_rows += rows;
    return RO_OK;
}

extern "C" int ro_stft_run_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                                    int64_t first_row, int64_t rows, float *d_rows, int64_t row_stride,
                                    float *d_tile, ro_scan_record_t *d_records, void *stream)
{
    return run_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile, d_records, nullptr, stream);
}

extern "C" int ro_stft_run_resident_sets(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                         int64_t rows, float *d_rows, int64_t row_stride, float *d_tile,
                                         ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream)
{
    return run_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile, d_records, d_extra, stream);
}

extern "C" int ro_stft_run_resident_ln(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                       int64_t rows, float *d_rows, int64_t row_stride, float *d_tile, float *d_ln_tile,
                                       float *d_ln_minmax, ro_scan_record_t *d_records, void *stream)
{
    int rc = validate_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile, d_records);
    if (rc != RO_OK || rows == 0) return rc;
    if (!h->cfg.tile_ln) return fail(RO_ERR_STATE, "this handle was not created with tile_ln");
    if (!d_tile) return fail(RO_ERR_INVALID, "the log image is cut from the tile: d_tile is required");
    if (d_ln_minmax && !d_ln_tile) return fail(RO_ERR_INVALID, "the range comes with the log image: pass d_ln_tile too");
    // (run_resident repeats validate_resident, which passes again, and sets the device)
    return run_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile, d_records, nullptr, stream,
                        d_ln_tile, d_ln_minmax);
}

extern "C" int ro_stft_spectra_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                                        int64_t first_row, int64_t rows, float *d_spectra, int64_t stride,
                                        void *stream)
{
    // same argument checks as the magnitude path (d_spectra in the place of d_rows)
    int rc = validate_resident(h, d_iq, format, samples, first_row, rows, d_spectra, stride, nullptr, nullptr);
    if (rc != RO_OK) return rc;
    if (h->czt) return fail(RO_ERR_UNSUPPORTED, "complex spectra are available for power-of-two bins");
    HIP_TRY(hipSetDevice(h->device));
    if (h->f64) {
        // the double transform itself, narrowed once per component (ro_f64reg.hip's SPEC instantiations): the register
        // kernel's sizes only
        if (!h->f64reg)
            return fail(RO_ERR_UNSUPPORTED, "complex spectra of RO_PRECISION_F64 handles are available up to 65536 bins");
        ro::F64RegArgs r = make_f64reg_args(h, d_iq, first_row, rows, d_spectra, stride);
        r.spectra = 1;
        HIP_TRY(ro::launch_f64reg(h->bins, format, r, (hipStream_t)stream));
        return RO_OK;
    }
    if (h->big)
        return launch_spectra_big(h, d_iq, format, first_row, rows, reinterpret_cast<float2 *>(d_spectra), stride,
                                  (hipStream_t)stream);
    ro::StftArgs a = make_stft_args(h, d_iq, first_row, rows, nullptr, 0);
    a.spec_out = reinterpret_cast<float2 *>(d_spectra);
    a.spec_stride = stride;
    HIP_TRY(ro::launch_stft(h->bins, format, a, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_stft_scan_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                     ro_scan_record_t *d_records, void *stream)
{
    if (!h || !d_rows || !d_records) return fail(RO_ERR_INVALID, "null argument");
    if (!h->cfg.enable_scan) return fail(RO_ERR_STATE, "scan bands not configured");
    if (rows < 0 || row_stride < h->bins) return fail(RO_ERR_INVALID, "bad rows / row_stride");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;      // NULL = the default (null) stream, like any HIP launch
    ro::ScanArgs sc = make_scan_args(h, d_rows, row_stride, rows, d_records);
    HIP_TRY(ro::launch_scan(sc, s));
    return RO_OK;
}

extern "C" int ro_stft_scan_sets_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                          ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream)
{
    if (!h || !d_rows || !d_extra) return fail(RO_ERR_INVALID, "null argument");
    if (!h->cfg.enable_scan) return fail(RO_ERR_STATE, "scan bands not configured");
    if (h->extra_count == 0) return fail(RO_ERR_STATE, "no extra band sets are set (ro_stft_set_extra_bands)");
    if (rows < 0 || row_stride < h->bins) return fail(RO_ERR_INVALID, "bad rows / row_stride");
    if (rows > (int64_t)0x0fffffff) return fail(RO_ERR_INVALID, "too many rows in one launch");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (d_records) HIP_TRY(ro::launch_scan(make_scan_args(h, d_rows, row_stride, rows, d_records), s));
    HIP_TRY(ro::launch_scan_sets(make_scan_sets_args(h, d_rows, row_stride, rows, d_extra), s));
    return RO_OK;
}

// ---------------------------------------------------------------------------
// tile windows: several recorders' column cuts of full rows (src/WaterfallBackend.cpp:174-205, :368-374) as one image
// ---------------------------------------------------------------------------
// what both calls ask of the window list and the image; *cut is ready for launch_tile_and_scan
static int check_cut(const char *who, const ro_stft_t *h, const ro_band_window_t *w, int count, const float *d_image,
                     int64_t image_stride, ro::CutArgs *cut)
{
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    if (!w || !d_image) return fail(RO_ERR_INVALID, "%s: null %s", who, !w ? "windows" : "d_image");
    int64_t total = 0;
    const int rc = tile_windows_check(who, h->bins, w, count, &total);
    if (rc != RO_OK) return rc;
    if (image_stride < total)
        return fail(RO_ERR_INVALID, "%s: image_stride %lld < the windows' %lld columns", who, (long long)image_stride,
                    (long long)total);
    *cut = make_cut_args(w, count, const_cast<float *>(d_image), image_stride);
    return RO_OK;
}

extern "C" int ro_stft_cut_windows_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                            const ro_band_window_t *w, int count, float *d_image, int64_t image_stride,
                                            void *stream)
{
    ro::CutArgs cut{};
    const int rc = check_cut("ro_stft_cut_windows_resident", h, w, count, d_image, image_stride, &cut);
    if (rc != RO_OK) return rc;
    if (!d_rows) return fail(RO_ERR_INVALID, "ro_stft_cut_windows_resident: null d_rows");
    if (rows < 0 || row_stride < h->bins) return fail(RO_ERR_INVALID, "bad rows / row_stride");
    if (rows == 0) return RO_OK;
    HIP_TRY(hipSetDevice(h->device));
    cut.rows_in = d_rows;
    cut.rows = rows;
    cut.row_stride = row_stride;
    HIP_TRY(ro::launch_cut_windows(cut, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_stft_run_resident_windows(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                            int64_t rows, float *d_rows, int64_t row_stride, const ro_band_window_t *w,
                                            int count, float *d_image, int64_t image_stride, ro_scan_record_t *d_records,
                                            ro_scan_record_t *d_extra, void *stream)
{
    ro::CutArgs cut{};
    const int rc = check_cut("ro_stft_run_resident_windows", h, w, count, d_image, image_stride, &cut);
    if (rc != RO_OK) return rc;
    return run_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, nullptr, d_records, d_extra, stream,
                        nullptr, nullptr, &cut);
}

// ---------------------------------------------------------------------------
// the detector on the device: events from scan records (src/BolidRecorder.cpp:135, :171-267; ro_events.hip)
// ---------------------------------------------------------------------------
// what both calls ask of the detector's arguments
static int check_events(const char *who, const ro_stft_t *h, const ro_scan_record_t *d_records, const ro_scan_record_t *d_extra,
                        int64_t rows, const ro_detector_t *detectors, const ro_detect_state_t *d_state,
                        const ro_event_t *d_events, int64_t capacity)
{
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    if (!d_state || !detectors) return fail(RO_ERR_INVALID, "%s: null %s", who, !d_state ? "d_state" : "detectors");
    if (!d_records && !d_extra) return fail(RO_ERR_INVALID, "%s: null d_records and null d_extra: one of them is needed", who);
    if (rows < 0 || capacity < 0)
        return fail(RO_ERR_INVALID, "%s: rows %lld, capacity %lld: neither may be negative", who, (long long)rows,
                    (long long)capacity);
    if (capacity > 0 && !d_events) return fail(RO_ERR_INVALID, "%s: null d_events with capacity %lld", who, (long long)capacity);
    if (d_extra && h->extra_count == 0)
        return fail(RO_ERR_STATE, "%s: d_extra, but no extra band sets are set (ro_stft_set_extra_bands)", who);
    for (int i = 0; i <= h->extra_count; ++i)
        if (detectors[i].advance < 0 || detectors[i].jitter < 0)
            return fail(RO_ERR_INVALID, "%s: set %d: advance %d, jitter %d: neither may be negative", who, i,
                        detectors[i].advance, detectors[i].jitter);
    return RO_OK;
}

// the launches (check_events has passed): chunks of RO_EVENTS_CHUNK_ROWS rows chained through d_state on the stream
static int launch_events_chunks(ro_stft_t *h, const ro_scan_record_t *d_records, const ro_scan_record_t *d_extra,
                                int64_t first_row, int64_t rows, const ro_detector_t *detectors, ro_detect_state_t *d_state,
                                ro_event_t *d_events, int64_t capacity, ro_detect_summary_t *d_summary, uint8_t *d_detect,
                                hipStream_t s)
{
    const int count = h->extra_count;
    if (rows == 0) {                             // nothing changes but the summaries of the slots asked for
        if (d_summary && d_records) HIP_TRY(hipMemsetAsync(d_summary, 0, sizeof(ro_detect_summary_t), s));
        if (d_summary && d_extra) HIP_TRY(hipMemsetAsync(d_summary + 1, 0, (size_t)count * sizeof(ro_detect_summary_t), s));
        return RO_OK;
    }
    if (!h->d_events_scratch) HIP_TRY(h->d_events_scratch.alloc(ro::EVENTS_SCRATCH_BYTES));
    ro::EventsArgs a{};
    ro::events_scratch_layout(a, h->d_events_scratch);
    a.count = count;
    a.state = d_state;
    a.events = d_events;
    a.capacity = capacity;
    a.summary = d_summary;
    for (int i = 0; i <= count; ++i) a.det[i] = detectors[i];
    for (int64_t done = 0; done < rows; done += RO_EVENTS_CHUNK_ROWS) {
        a.primary = d_records ? d_records + done : nullptr;
        a.extra = d_extra ? d_extra + done * count : nullptr;
        a.accumulate = done > 0;
        a.first_row = first_row + done;
        a.rows = std::min<int64_t>(RO_EVENTS_CHUNK_ROWS, rows - done);
        a.detect = d_detect ? d_detect + done * (1 + count) : nullptr;
        HIP_TRY(ro::launch_events(a, s));
    }
    return RO_OK;
}

extern "C" int ro_stft_events_resident(ro_stft_t *h, const ro_scan_record_t *d_records, const ro_scan_record_t *d_extra,
                                       int64_t first_row, int64_t rows, const ro_detector_t *detectors,
                                       ro_detect_state_t *d_state, ro_event_t *d_events, int64_t capacity,
                                       ro_detect_summary_t *d_summary, uint8_t *d_detect, void *stream)
{
    const int rc = check_events("ro_stft_events_resident", h, d_records, d_extra, rows, detectors, d_state, d_events, capacity);
    if (rc != RO_OK) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return launch_events_chunks(h, d_records, d_extra, first_row, rows, detectors, d_state, d_events, capacity, d_summary,
                                d_detect, (hipStream_t)stream);
}

extern "C" int ro_stft_run_resident_events(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                           int64_t rows, float *d_rows, int64_t row_stride, float *d_tile,
                                           ro_scan_record_t *d_records, ro_scan_record_t *d_extra,
                                           const ro_detector_t *detectors, ro_detect_state_t *d_state, ro_event_t *d_events,
                                           int64_t capacity, ro_detect_summary_t *d_summary, uint8_t *d_detect, void *stream)
{
    int rc = check_events("ro_stft_run_resident_events", h, d_records, d_extra, rows, detectors, d_state, d_events, capacity);
    if (rc != RO_OK) return rc;
    rc = run_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile, d_records, d_extra, stream);
    if (rc != RO_OK) return rc;
    return launch_events_chunks(h, d_records, d_extra, first_row, rows, detectors, d_state, d_events, capacity, d_summary,
                                d_detect, (hipStream_t)stream);
}

extern "C" int ro_stft_extra_bands(const ro_stft_t *h, ro_bands_t *sets_out)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    if (sets_out)
        for (int i = 0; i < h->extra_count; ++i) sets_out[i] = h->extra[i];
    return h->extra_count;
}

extern "C" int ro_stft_ln_tile_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                        int first_col, int cols, float *d_ln, uint8_t *d_u8, float *d_minmax,
                                        void *stream)
{
    if (!h || !d_rows) return fail(RO_ERR_INVALID, "null argument");
    if (!d_ln && !d_u8 && !d_minmax) return fail(RO_ERR_INVALID, "no output requested");
    if (rows < 0 || row_stride < h->bins) return fail(RO_ERR_INVALID, "bad rows / row_stride");
    if (first_col < 0 || cols <= 0 || (int64_t)first_col + cols > h->bins)
        return fail(RO_ERR_INVALID, "columns outside the row");
    HIP_TRY(hipSetDevice(h->device));
    ro::LnArgs a;
    a.rows_in = d_rows;
    a.ln_out = d_ln;
    a.u8_out = d_u8;
    a.keys = h->d_ln_keys + 2 * (h->ln_calls++ & 15);      // a pair of its own for each of 16 calls in flight
    a.minmax = d_minmax;
    a.rows = rows;
    a.row_stride = row_stride;
    a.first = first_col;
    a.cols = cols;
    HIP_TRY(ro::launch_ln_tile(a, (hipStream_t)stream));
    return RO_OK;
}

// ---------------------------------------------------------------------------
// band-only transform
// ---------------------------------------------------------------------------
extern "C" int ro_stft_band_supported(int bins, int cols)
{
    ro::BandPlan p;
    return ro::band_plan(bins, cols, p) ? 1 : 0;
}

extern "C" int ro_stft_band_supported_precision(int bins, int cols, int precision)
{
    if (precision == RO_PRECISION_F32) return ro_stft_band_supported(bins, cols);
    if (precision != RO_PRECISION_F64) return 0;
    ro::Band64Plan p;
    return ro::band64_plan(bins, cols, p) ? 1 : 0;
}

extern "C" int ro_bands_hull(const ro_bands_t *b, int bins, int tile_first_col, int tile_cols, int *first_col, int *cols)
{
    if (!b || !first_col || !cols) return fail(RO_ERR_INVALID, "ro_bands_hull: null argument");
    if (b->noise_width <= 0 || b->detect_width <= 0 || b->avg_bins <= 0)
        return fail(RO_ERR_INVALID, "bands: widths and avg_bins must be positive");
    if (tile_cols < 0) return fail(RO_ERR_INVALID, "tile_cols must not be negative");
    // average() reads avg_bins columns from low_detect + peak - avg_bins / 2, peak in [0, detect_width)
    // (src/BolidRecorder.cpp:126-132)
    int64_t lo = std::min<int64_t>(b->low_noise, (int64_t)b->low_detect - b->avg_bins / 2);
    int64_t hi = std::max<int64_t>((int64_t)b->low_noise + b->noise_width,
                                   (int64_t)b->low_detect + b->detect_width - 1 - b->avg_bins / 2 + b->avg_bins);
    if (tile_cols > 0) {
        lo = std::min<int64_t>(lo, tile_first_col);
        hi = std::max<int64_t>(hi, (int64_t)tile_first_col + tile_cols);
    }
    if (lo < 0 || hi > bins)
        return fail(RO_ERR_INVALID, "what the recorders read, columns [%lld,%lld), leaves the row [0,%d)", (long long)lo,
                    (long long)hi, bins);
    *first_col = (int)lo;
    *cols = (int)(hi - lo);
    return RO_OK;
}

namespace {

// exp(-2 pi i e / n) for an exactly reduced integer phase e in [0, n): the float tables' evaluated in double and narrowed
// once, the double tables' evaluated in long double and rounded once
void unit_root(int64_t e, int64_t n, float2 &out)
{
    const double ang = -2.0 * M_PI * (double)e / (double)n;
    out = make_float2((float)cos(ang), (float)sin(ang));
}
void unit_root(int64_t e, int64_t n, double2 &out)
{
    const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)e / (long double)n;
    out = make_double2((double)cosl(ang), (double)sinl(ang));
}

// the tables of the columns the windows list (image column j = the j-th column of the list, bin k(j)), uploaded on first
// use and kept until another list is asked for
template <typename T, typename Plan>
int ensure_band_tables(ro_stft *h, BandState<T> &st, const Plan &p, const ro_band_window_t *w, int count)
{
    if ((int)h->band_key.size() == count &&
        std::equal(w, w + count, h->band_key.begin(), [](const ro_band_window_t &x, const ro_band_window_t &y) {
            return x.first_col == y.first_col && x.cols == y.cols;
        }))
        return RO_OK;
    if (st.tw || st.t1 || st.t2 || st.kcell) HIP_TRY(hipDeviceSynchronize());     // an earlier launch may still be reading the old tables
    st.tw.reset();                                      // (all four, whichever a failed call before this one left behind)
    st.t1.reset();
    st.t2.reset();
    st.kcell.reset();
    h->band_key.clear();
    const int64_t n = h->bins;
    std::vector<int64_t> ks;                            // the bins, in image order
    for (int i = 0; i < count; ++i)
        for (int c = 0; c < w[i].cols; ++c) ks.push_back(((int64_t)w[i].first_col + c + n / 2) % n);
    const int cols = (int)ks.size();
    std::vector<T> tw((size_t)p.m), t1((size_t)cols * p.a), t2((size_t)p.slabs * cols);
    std::vector<int32_t> kcell((size_t)cols);
    for (int j = 0; j < p.m; ++j) unit_root(j, p.m, tw[(size_t)j]);
    for (int j = 0; j < cols; ++j) {
        const int64_t k = ks[(size_t)j];
        kcell[(size_t)j] = ro::band_cell(p.m, (int)(k % p.m)) * p.a;          // < a m: inside the workgroup's LDS image
                                                                              // (read by the window-list kernels only)
        for (int t = 0; t < p.a; ++t) unit_root((t * k) % n, n, t1[(size_t)j * p.a + t]);
        for (int s = 0; s < p.slabs; ++s) unit_root(((int64_t)s * p.a * k) % n, n, t2[(size_t)s * cols + j]);
    }
    HIP_TRY(st.tw.upload(tw));
    HIP_TRY(st.t1.upload(t1));
    HIP_TRY(st.t2.upload(t2));
    HIP_TRY(st.kcell.upload(kcell));
    h->band_key.assign(w, w + count);
    return RO_OK;
}

// how each kernel family is told which columns the image shows: the consecutive call's kernels (ro_band.hip,
// ro_band_f64.hip) derive the bins from first_col, the window-list kernels read the table
inline void set_columns(ro::BandArgs &b, const ro_band_window_t *w, const int32_t *) { b.first_col = w[0].first_col; }
inline void set_columns(ro::Band64Args &b, const ro_band_window_t *w, const int32_t *) { b.first_col = w[0].first_col; }
inline void set_columns(ro::BandWinArgs &b, const ro_band_window_t *, const int32_t *kcell) { b.kcell = kcell; }
inline void set_columns(ro::Band64WinArgs &b, const ro_band_window_t *, const int32_t *kcell) { b.kcell = kcell; }

// rows [first_row, +rows) of the `cols` columns the windows list, in one precision and one kernel family (Args =
// ro::BandArgs with launch_band, ro::Band64Args with launch_band64: one window; ro::BandWinArgs with launch_band_windows,
// ro::Band64WinArgs with launch_band64_windows: any list): the tables, the partial sums, the launches chunk by chunk, the
// scans of the band image, the counters
template <typename Args, typename T, typename Plan, typename Launch>
int run_band(ro_stft *h, BandState<T> &st, const Plan &p, Launch launch, const void *d_iq, int format, int64_t first_row,
             int64_t rows, const ro_band_window_t *w, int count, int cols, float *d_band, int64_t band_stride,
             const ro::ScanArgs *sc, const ro::ScanSetsArgs *ss, hipStream_t s)
{
    int rc = ensure_band_tables(h, st, p, w, count);
    if (rc != RO_OK) return rc;
    // the partial sums: rows per chunk like the large transforms' scratch, 256 MiB at the most, one grid of <= 65535 rows
    const size_t row_bytes = (size_t)p.slabs * cols * sizeof(T);
    const int64_t chunk = std::min<int64_t>(std::min<int64_t>(rows, 65535),
                                            std::max<int64_t>(1, (int64_t)(((size_t)256 << 20) / row_bytes)));
    if ((size_t)chunk * row_bytes > st.part_bytes) {
        if (st.part) HIP_TRY(hipDeviceSynchronize());   // (an earlier launch may still be using the old block)
        st.part_bytes = 0;
        HIP_TRY(st.part.alloc((size_t)chunk * row_bytes / sizeof(T)));
        st.part_bytes = (size_t)chunk * row_bytes;
    }
    for (int64_t done = 0; done < rows; done += chunk) {
        Args b{};
        b.iq = d_iq;
        b.window = h->d_window;
        b.tw = st.tw;
        b.t1 = st.t1;
        b.t2 = st.t2;
        set_columns(b, w, st.kcell);
        b.part = st.part;
        b.band_out = d_band + done * band_stride;
        b.first_row = first_row + done;
        b.rows = std::min(chunk, rows - done);
        b.band_stride = band_stride;
        b.hop = h->hop;
        b.bins = h->bins;
        b.cols = cols;
        b.gain = (decltype(b.gain))h->cfg.iq_gain;
        HIP_TRY(launch(p, format, b, s));
    }
    if (sc) HIP_TRY(ro::launch_scan(*sc, s));
    if (ss) HIP_TRY(ro::launch_scan_sets(*ss, s));
    h->stat_launches += 1;
    h->stat_rows += rows;
    return RO_OK;
}

// what both band calls refuse about the handle and the sample format, before they look at the columns
int check_band_handle(const ro_stft *h, int format)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    if (h->czt) return fail(RO_ERR_UNSUPPORTED, "the band-only transform needs power-of-two bins (got %d)", h->bins);
    if (h->f64 && h->bins < 131072)
        return fail(RO_ERR_UNSUPPORTED, "the band-only transform of RO_PRECISION_F64 handles starts at 131072 bins (got %d): "
                                        "up to 65536 the full row comes from registers without scratch", h->bins);
    if (format == RO_IQ_F64 && !h->f64)
        return fail(RO_ERR_UNSUPPORTED, "the band-only transform takes RO_IQ_F32 or RO_IQ_I16 samples "
                                        "(RO_IQ_F64 on RO_PRECISION_F64 handles of 131072 bins and above)");
    if (format != RO_IQ_F32 && format != RO_IQ_I16 && format != RO_IQ_F64)
        return fail(RO_ERR_INVALID, "resident input must be RO_IQ_F32, RO_IQ_I16 or RO_IQ_F64 (got %d)", format);
    return RO_OK;
}

// ... and what they refuse once the columns and the scans are settled; *go = false: rows == 0, RO_OK and nothing to do
int check_band_input(const ro_stft *h, const void *d_iq, int64_t samples, int64_t first_row, int64_t rows,
                     const float *d_band, bool *go)
{
    *go = false;
    if (rows == 0) return RO_OK;
    if (!d_iq) return fail(RO_ERR_INVALID, "null input pointer");
    if (!d_band) return fail(RO_ERR_INVALID, "d_band is required");
    const int64_t last = (first_row + rows - 1) * (int64_t)h->hop + h->bins;
    if (last > samples)
        return fail(RO_ERR_INVALID, "rows [%lld,+%lld) need %lld samples, buffer holds %lld", (long long)first_row,
                    (long long)rows, (long long)last, (long long)samples);
    if (rows > (int64_t)0x0fffffff) return fail(RO_ERR_INVALID, "too many rows in one launch");
    *go = true;
    return RO_OK;
}

// the two intervals a band set reads of a row: its noise band, and its detect band widened by what average() reads around
// any peak (ro_bands_hull has the sources)
struct SetReads { int64_t noise_lo, noise_hi, detect_lo, detect_hi; };
SetReads set_reads(const ro_bands_t &b)
{
    return {b.low_noise, (int64_t)b.low_noise + b.noise_width, (int64_t)b.low_detect - b.avg_bins / 2,
            (int64_t)b.low_detect + b.detect_width - 1 - b.avg_bins / 2 + b.avg_bins};
}

// the window that holds columns [lo, hi) whole, and where it starts in the image; -1: none
int window_of(const ro_band_window_t *w, int count, int64_t lo, int64_t hi, int *image_off)
{
    int off = 0;
    for (int i = 0; i < count; ++i) {
        if (lo >= w[i].first_col && hi <= (int64_t)w[i].first_col + w[i].cols) {
            *image_off = off;
            return i;
        }
        off += w[i].cols;
    }
    return -1;
}

// band set `b` (set `index`: 0 the primary, 1 ... the extras) in image coordinates, or RO_ERR_INVALID
int move_set(const ro_band_window_t *w, int count, const ro_bands_t &b, int index, ro_bands_t &out)
{
    const SetReads r = set_reads(b);
    int off_n = 0, off_d = 0;
    const int wn = window_of(w, count, r.noise_lo, r.noise_hi, &off_n);
    if (wn < 0)
        return fail(RO_ERR_INVALID, "records of band set %d need its noise band, columns [%lld,%lld), inside one window",
                    index, (long long)r.noise_lo, (long long)r.noise_hi);
    const int wd = window_of(w, count, r.detect_lo, r.detect_hi, &off_d);
    if (wd < 0)
        return fail(RO_ERR_INVALID, "records of band set %d need its detect band and the average's margin, columns "
                                    "[%lld,%lld), inside one window", index, (long long)r.detect_lo, (long long)r.detect_hi);
    out = b;
    out.low_noise = b.low_noise - w[wn].first_col + off_n;
    out.low_detect = b.low_detect - w[wd].first_col + off_d;
    return RO_OK;
}

// 0: valid; otherwise why not (total: the columns in all, also when they are too many)
const char *windows_fault(int bins, const ro_band_window_t *w, int count, int64_t *total)
{
    *total = 0;
    if (!w) return "null windows";
    if (count < 1 || count > RO_MAX_BAND_WINDOWS) return "a call takes 1 ... 8 windows";
    for (int i = 0; i < count; ++i) {
        if (w[i].cols < 1) return "every window needs at least one column";
        if (w[i].first_col < 0 || (int64_t)w[i].first_col + w[i].cols > bins) return "a window lies outside the row";
        if (i > 0 && w[i].first_col < (int64_t)w[i - 1].first_col + w[i - 1].cols)
            return "the windows must be ascending and must not overlap";
        *total += w[i].cols;
    }
    return nullptr;
}

}  // namespace

extern "C" int ro_stft_band_windows_supported(int bins, const ro_band_window_t *w, int count, int precision)
{
    int64_t total = 0;
    if (bins < 1 || windows_fault(bins, w, count, &total) || total > 1024) return 0;
    return ro_stft_band_supported_precision(bins, (int)total, precision);
}

extern "C" int ro_bands_windows(const ro_bands_t *sets, int set_count, int bins, int tile_first_col, int tile_cols,
                                ro_band_window_t *windows_out, int *count_out)
{
    if (!sets || !windows_out || !count_out) return fail(RO_ERR_INVALID, "ro_bands_windows: null argument");
    if (set_count < 1 || set_count > 1 + RO_MAX_EXTRA_BANDS)
        return fail(RO_ERR_INVALID, "%d band sets: 1 ... %d (a primary and its extras)", set_count, 1 + RO_MAX_EXTRA_BANDS);
    if (tile_cols < 0) return fail(RO_ERR_INVALID, "tile_cols must not be negative");
    std::vector<std::pair<int64_t, int64_t>> iv;        // [lo, hi)
    for (int i = 0; i < set_count; ++i) {
        const ro_bands_t &b = sets[i];
        if (b.noise_width <= 0 || b.detect_width <= 0 || b.avg_bins <= 0)
            return fail(RO_ERR_INVALID, "bands: widths and avg_bins must be positive");
        const SetReads r = set_reads(b);
        iv.emplace_back(r.noise_lo, r.noise_hi);
        iv.emplace_back(r.detect_lo, r.detect_hi);
    }
    if (tile_cols > 0) iv.emplace_back(tile_first_col, (int64_t)tile_first_col + tile_cols);
    for (const auto &x : iv)
        if (x.first < 0 || x.second > bins)
            return fail(RO_ERR_INVALID, "what the recorders read, columns [%lld,%lld), leaves the row [0,%d)",
                        (long long)x.first, (long long)x.second, bins);
    std::sort(iv.begin(), iv.end());
    std::vector<std::pair<int64_t, int64_t>> m;
    for (const auto &x : iv) {
        if (!m.empty() && x.first <= m.back().second) m.back().second = std::max(m.back().second, x.second);
        else m.push_back(x);
    }
    while ((int)m.size() > RO_MAX_BAND_WINDOWS) {       // the smallest gap goes; the lower pair on a tie
        size_t best = 0;
        for (size_t i = 1; i + 1 < m.size(); ++i)
            if (m[i + 1].first - m[i].second < m[best + 1].first - m[best].second) best = i;
        m[best].second = m[best + 1].second;
        m.erase(m.begin() + (std::ptrdiff_t)best + 1);
    }
    for (size_t i = 0; i < m.size(); ++i) {
        windows_out[i].first_col = (int32_t)m[i].first;
        windows_out[i].cols = (int32_t)(m[i].second - m[i].first);
    }
    *count_out = (int)m.size();
    return RO_OK;
}

extern "C" int ro_stft_band_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                     int64_t rows, int first_col, int cols, float *d_band, int64_t band_stride,
                                     ro_scan_record_t *d_records, void *stream)
{
    int rc = check_band_handle(h, format);
    if (rc != RO_OK) return rc;
    ro::BandPlan p{};
    ro::Band64Plan p64{};
    if (h->f64 ? !ro::band64_plan(h->bins, cols, p64) : !ro::band_plan(h->bins, cols, p))
        return fail(RO_ERR_UNSUPPORTED, "no band kernel for %d columns of %d bins (bins a power of two %d ... 1048576, "
                                        "1 ... 1024 columns)", cols, h->bins, h->f64 ? 131072 : 16384);
    if (first_col < 0 || (int64_t)first_col + cols > h->bins)
        return fail(RO_ERR_INVALID, "band [%d,+%d) outside [0,%d)", first_col, cols, h->bins);
    if (band_stride < cols) return fail(RO_ERR_INVALID, "band_stride %lld < cols %d", (long long)band_stride, cols);
    if (rows < 0 || first_row < 0) return fail(RO_ERR_INVALID, "negative row range");
    ro::ScanArgs sc{};
    if (d_records) {
        if (!h->cfg.enable_scan) return fail(RO_ERR_INVALID, "records requested but enable_scan == 0");
        int lo = 0, n = 0;
        rc = ro_bands_hull(&h->cfg.bands, h->bins, 0, 0, &lo, &n);
        if (rc != RO_OK) return rc;
        if (lo < first_col || lo + n > first_col + cols)
            return fail(RO_ERR_INVALID, "records need columns [%d,%d) (the bands and the average's margin); the band is [%d,%d)",
                        lo, lo + n, first_col, first_col + cols);
        // the scan kernel of the full rows on the band image: the band is its row, the bands move by first_col
        // (peak counts from low_detect and stays what it is)
        sc = make_scan_args(h, d_band, band_stride, rows, d_records);
        sc.bins = cols;
        sc.low_noise -= first_col;
        sc.low_detect -= first_col;
    }
    bool go = false;
    rc = check_band_input(h, d_iq, samples, first_row, rows, d_band, &go);
    if (!go) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const ro::ScanArgs *scan = d_records ? &sc : nullptr;
    const ro_band_window_t one = {first_col, cols};
    if (h->f64)
        return run_band<ro::Band64Args>(h, h->band64, p64, ro::launch_band64, d_iq, format, first_row, rows, &one, 1, cols,
                                        d_band, band_stride, scan, nullptr, s);
    return run_band<ro::BandArgs>(h, h->band, p, ro::launch_band, d_iq, format, first_row, rows, &one, 1, cols, d_band,
                                  band_stride, scan, nullptr, s);
}

extern "C" int ro_stft_band_windows_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row,
                                             int64_t rows, const ro_band_window_t *w, int count, float *d_band,
                                             int64_t band_stride, ro_scan_record_t *d_records, ro_scan_record_t *d_extra,
                                             void *stream)
{
    int rc = check_band_handle(h, format);
    if (rc != RO_OK) return rc;
    int64_t total = 0;
    if (const char *why = windows_fault(h->bins, w, count, &total))
        return fail(RO_ERR_INVALID, "band windows: %s (%d windows of a %d-bin row)", why, count, h->bins);
    ro::BandPlan p{};
    ro::Band64Plan p64{};
    if (total > 1024 || (h->f64 ? !ro::band64_plan(h->bins, (int)total, p64) : !ro::band_plan(h->bins, (int)total, p)))
        return fail(RO_ERR_UNSUPPORTED, "no band kernel for %lld columns of %d bins (bins a power of two %d ... 1048576, "
                                        "1 ... 1024 columns in all)", (long long)total, h->bins, h->f64 ? 131072 : 16384);
    const int cols = (int)total;
    if (band_stride < cols)
        return fail(RO_ERR_INVALID, "band_stride %lld < the windows' %d columns", (long long)band_stride, cols);
    if (rows < 0 || first_row < 0) return fail(RO_ERR_INVALID, "negative row range");
    // the scan kernels of the full rows on the band image: the image is their row, each band moves to where its window
    // sits in it (peak counts from low_detect and stays what it is)
    ro::ScanArgs sc{};
    ro::ScanSetsArgs ss{};
    if (d_records) {
        if (!h->cfg.enable_scan) return fail(RO_ERR_INVALID, "records requested but enable_scan == 0");
        ro_bands_t moved{};
        rc = move_set(w, count, h->cfg.bands, 0, moved);
        if (rc != RO_OK) return rc;
        sc = make_scan_args(h, d_band, band_stride, rows, d_records);
        sc.bins = cols;
        sc.low_noise = moved.low_noise;
        sc.low_detect = moved.low_detect;
    }
    if (d_extra) {
        // (extra sets exist only on a handle that scans: ro_stft_set_extra_bands refuses them without enable_scan, so
        // extra_count > 0 implies it, as on the full path)
        if (h->extra_count == 0)
            return fail(RO_ERR_STATE, "extra records requested but no extra band sets are set (ro_stft_set_extra_bands)");
        ss = make_scan_sets_args(h, d_band, band_stride, rows, d_extra);
        ss.bins = cols;
        for (int i = 0; i < h->extra_count; ++i) {
            rc = move_set(w, count, h->extra[i], 1 + i, ss.sets[i]);
            if (rc != RO_OK) return rc;
        }
    }
    bool go = false;
    rc = check_band_input(h, d_iq, samples, first_row, rows, d_band, &go);
    if (!go) return rc;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    const ro::ScanArgs *scan = d_records ? &sc : nullptr;
    const ro::ScanSetsArgs *sets = d_extra ? &ss : nullptr;
    if (h->f64)
        return run_band<ro::Band64WinArgs>(h, h->band64, p64, ro::launch_band64_windows, d_iq, format, first_row, rows, w,
                                           count, cols, d_band, band_stride, scan, sets, s);
    return run_band<ro::BandWinArgs>(h, h->band, p, ro::launch_band_windows, d_iq, format, first_row, rows, w, count, cols,
                                     d_band, band_stride, scan, sets, s);
}

extern "C" int ro_stft_time_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                                     int64_t first_row, int64_t rows, float *d_rows, int64_t row_stride,
                                     float *d_tile, ro_scan_record_t *d_records, void *stream, int iters,
                                     float *ms_out, float *kernel_ms_out)
{
    int rc = validate_resident(h, d_iq, format, samples, first_row, rows, d_rows, row_stride, d_tile,
                               d_records);
    if (rc != RO_OK) return rc;
    if (iters <= 0 || !ms_out) return fail(RO_ERR_INVALID, "iters must be positive and ms_out non-null");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;      // NULL = the default (null) stream, like any HIP launch
    std::vector<hipEvent_t> ev((size_t)iters * 3, nullptr);
    for (auto &e : ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            for (auto &d : ev) if (d) (void)hipEventDestroy(d);
            return fail(RO_ERR_HIP, "hipEventCreate failed");
        }
    }
    for (int i = 0; i < iters && rc == RO_OK; ++i) {
        hipError_t e = hipEventRecord(ev[3 * i], s);
        if (e == hipSuccess) {
            rc = launch_transform(h, d_iq, format, first_row, rows, d_rows, row_stride, s, d_tile, d_records);
            if (rc != RO_OK) break;
            e = hipEventRecord(ev[3 * i + 1], s);
        }
        if (e == hipSuccess) {
            rc = launch_tile_and_scan(h, d_rows, row_stride, rows, d_tile, d_records, s);
            if (rc != RO_OK) break;
            e = hipEventRecord(ev[3 * i + 2], s);
        }
        if (e != hipSuccess) rc = fail(RO_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
    }
    if (rc != RO_OK) {                                  // leave no event behind on the error paths
        (void)hipStreamSynchronize(s);
        for (auto &e : ev) (void)hipEventDestroy(e);
        return rc;
    }
    hipError_t es = hipStreamSynchronize(s);
    double k0 = 0.0, k1 = 0.0;
    for (int i = 0; i < iters && es == hipSuccess; ++i) {
        float t = 0.f, t0 = 0.f, t1 = 0.f;
        if ((es = hipEventElapsedTime(&t, ev[3 * i], ev[3 * i + 2])) != hipSuccess) break;
        if ((es = hipEventElapsedTime(&t0, ev[3 * i], ev[3 * i + 1])) != hipSuccess) break;
        if ((es = hipEventElapsedTime(&t1, ev[3 * i + 1], ev[3 * i + 2])) != hipSuccess) break;
        ms_out[i] = t;
        k0 += t0;
        k1 += t1;
    }
    if (es != hipSuccess) {
        for (auto &e : ev) (void)hipEventDestroy(e);
        return fail(RO_ERR_HIP, "timing the resident path failed: %s", hipGetErrorString(es));
    }
    if (kernel_ms_out) {
        kernel_ms_out[0] = (float)(k0 / iters);
        kernel_ms_out[1] = (float)(k1 / iters);
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    h->stat_launches += iters;
    h->stat_rows += rows * (int64_t)iters;
    return RO_OK;
}

extern "C" int ro_stft_timing(ro_stft_t *h, ro_stft_timing_t *out, int reset)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    if (out) {
        *out = h->timing;
        out->push_ms_avg = h->timing.push_calls ? h->push_ms_sum / (double)h->timing.push_calls : 0.0;
        out->batch_gpu_ms_avg = h->timed_batches ? h->batch_ms_sum / (double)h->timed_batches : 0.0;
        out->row_gpu_us_avg = h->timed_rows ? h->batch_ms_sum * 1e3 / (double)h->timed_rows : 0.0;
        out->fetch_ms_avg = h->timing.fetch_calls ? h->fetch_ms_sum / (double)h->timing.fetch_calls : 0.0;
    }
    if (reset) {                                             // FFTBackend::clearProcessingTime, src/FFTBackend.h:231-235
        h->timing = ro_stft_timing_t{};
        h->push_ms_sum = h->batch_ms_sum = h->fetch_ms_sum = 0.0;
        h->timed_batches = h->timed_rows = 0;
    }
    return RO_OK;
}

extern "C" int ro_stft_stats(const ro_stft_t *h, int64_t *samples_in, int64_t *rows_out, int64_t *launches,
                             double *kernel_ms_total)
{
    if (!h) return fail(RO_ERR_INVALID, "null handle");
    if (samples_in) *samples_in = h->stat_samples;
    if (rows_out) *rows_out = h->stat_rows;
    if (launches) *launches = h->stat_launches;
    if (kernel_ms_total) *kernel_ms_total = h->stat_kernel_ms;
    return RO_OK;
}
