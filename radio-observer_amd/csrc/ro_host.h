// ro_host.h -- what the translation units behind the C ABI share (internal; include/ro_stft.h is the ABI):
// the handle, the batches of the streaming path, the error text and the entry points one file offers the others.
//   ro_abi_helpers.cpp   error text, FFTBackend's public arithmetic, window tables, shard arithmetic, pinned memory
//   ro_exchange.cpp      the RCCL stitch of sharded rows (all-gather, gather to one rank, direct exchange)
//   ro_stream.cpp        push / flush / fetch: staging slots, captured graphs, the row sink
//   ro_czt.cpp           lengths that are not a power of two (chirp-z on an inner handle)
//   ro_stft_capi.cpp     create / destroy, the transform launches, the resident entry points
//   ro_snapshots.cpp     the row ring and the event snapshots cut from it (ro_snapshots.hip), and their host twin
//   ro_raw.cpp           the raw I/Q of each event, cut from the resident samples (ro_raw.hip), and its host twin
//   ro_units.cpp         the events' files as FITS data units (ro_units.hip), and their host twins
//   ro_periodic.cpp      the periodic snapshots' plan (host arithmetic), their data units cut from the ring (ro_periodic.hip)
//                        and the host twin
//   ro_levels.cpp        the grey-level previews of the event snapshots and of the periodic snapshots (ro_levels.hip), and
//                        their host twins
//   ro_png.cpp           the level images as complete PNG files (ro_png.hip), the one file writer of the host and the host
//                        twins of both kinds of file over it, and a periodic plan's directory in level form
//   ro_png_deflate.cpp   the same files with Huffman-coded deflate blocks (ro_png_deflate.hip), and a block's code and its
//                        bytes on the host, in either form
//   ro_resize.cpp        the level images resized to a width, Pillow's Lanczos to the byte (ro_resize.hip): the plan with
//                        its tap tables (host arithmetic), the launches, and the host twin
// Said once, here: pack_walk, the walk of every host twin that packs a source directory into a buffer (the units, the level
// images, both kinds of file), and scratch_for (ro_stft_capi.cpp), the prelude of every plan-then-copy call.
// ro_owned.h has the type that owns every device and pinned block of the handle, its slots and its batches.
// There is no CPU compute path in any of them: rows only ever come out of the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <deque>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/ro_stft.h"
#include "ro_kernels.h"
#include "ro_band.h"
#include "ro_band_f64.h"
#include "ro_band_windows.h"
#include "ro_events.h"
#include "ro_snapshots.h"
#include "ro_raw.h"
#include "ro_units.h"
#include "ro_periodic.h"
#include "ro_levels.h"
#include "ro_png.h"
#include "ro_png_deflate.h"
#include "ro_resize.h"
#include "ro_narrow.h"
#include "ro_owned.h"

// a -DRO_DIAG=1 build (tools/ab_build.sh) reads its run-time knobs (RO_BIG_FORM, RO_F64_SCRATCH_MB) from the environment
#if defined(RO_DIAG) && !defined(RO_DIAG_KNOBS)
#define RO_DIAG_KNOBS 1
#endif

// scratch of the large transforms' scratch form (the folded sub-rows between the kernels), MiB per block
#ifndef RO_SPEC_SCRATCH_MB
#define RO_SPEC_SCRATCH_MB 2048
#endif
// the four-step form's scratch (one block of Z between its two kernels), MiB AT MOST: the block grows to what a
// launch asks for (a streaming handle at Ionozor's shape launches a handful of rows and holds a few MiB, not the
// limit).  1 GiB measured best for resident launches -- blocks inside the 256 MiB Infinity Cache were 3 % faster for the
// row kernel and 13 % slower for the column kernel (profiles/r04_fourstep.txt).  Diagnostic builds: RO_FOUR_SCRATCH_MB
#ifndef RO_FOUR_SCRATCH_MB
#define RO_FOUR_SCRATCH_MB 1024
#endif
// RO_PRECISION_F64: MiB per complex-double scratch block (two blocks); the passes of one chunk run back to back, and a
// chunk that stays inside the 256 MiB Infinity Cache keeps most of the trip between them off HBM: 2.75-2.87 x 10^6
// rows/s at the C3 shape with 128 against 2.46 with 512, 2.36 with 256, 2.50 with 64, 1.96 with 32 (too few workgroups
// per launch); the same bits whatever the chunk (profiles/r04_strict_chunk.txt, tools/r4/strict_sweep.py)
#ifndef RO_F64_SCRATCH_MB
#define RO_F64_SCRATCH_MB 128
#endif
// RO_PRECISION_F64_ONE_LAUNCH (ro_f64fused.hip): a ring of this many rows of 32768 bins per XCD (scaled so that the
// ring's bytes stay the same at the other sizes), this many workgroups per CU.  4 rows is the least that keeps an XCD's
// 32 workgroups busy, and all its L2 serves (profiles/r05_f64_one_launch.txt)
#ifndef RO_F64_RING_ROWS
#define RO_F64_RING_ROWS 4
#endif
#ifndef RO_F64_WGS_PER_CU
#define RO_F64_WGS_PER_CU 1
#endif
// streaming path: sets of device + pinned staging buffers a handle rotates through (batches that can be in flight at once)
#ifndef RO_STREAM_SLOTS
#define RO_STREAM_SLOTS 3
#endif
// streaming path: a full latency-bound batch with a row sink runs as one captured graph per slot (run_stream_batch)
#ifndef RO_STREAM_GRAPH
#define RO_STREAM_GRAPH 1
#endif
// ... whose timing events go round one batch in this many (run_stream_batch has the measurement)
#ifndef RO_GRAPH_TIME_EVERY
#define RO_GRAPH_TIME_EVERY 8
#endif

namespace ro {
namespace host {

// RO_ERR_* code in, the same code out; the text is what ro_last_error() returns on this thread
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *last_error_text();

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess)                                                             \
            return fail(RO_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

inline double now_ms()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

// One launch worth of finished rows on their way to the caller.  The buffers are pinned host
// memory (hipHostMalloc) recycled through a free list; `done` fires when the device-to-host
// copies have landed, so ro_stft_push never waits for the GPU -- only ro_stft_fetch does.
struct Batch {
    int64_t first_row = 0;
    int64_t rows = 0;
    PinnedBlock<float> data;                   // capacity_rows x out_cols
    PinnedBlock<float> ln;                     // capacity_rows x out_cols (tile_ln)
    PinnedBlock<float> minmax;                 // capacity_rows x 2 (tile_ln)
    PinnedBlock<ro_scan_record_t> records;     // capacity_rows
    PinnedBlock<ro_scan_record_t> extra;       // capacity_rows x extra_count (extra band sets)
    int64_t capacity_rows = 0;
    int64_t consumed = 0;                      // rows already fetched
    hipEvent_t done = nullptr;
    hipEvent_t k0 = nullptr, k1 = nullptr;     // around the kernels of this batch (timing counters)
    bool pending = false;                      // `done` not yet waited for
    bool timed = true;                         // k0 / k1 were recorded around this batch's kernels
};

// the band-only transform's device state in one precision (T = float2: ro_band.hip, double2: ro_band_f64.hip): the tables
// of the last column windows asked for and the slabs' partial sums between the two kernels, grown on demand
template <typename T>
struct BandState {
    DeviceBlock<T> tw;                         // [m]: exp(-2 pi i j / m)
    DeviceBlock<T> t1;                         // [cols][a]: exp(-2 pi i t k / bins)
    DeviceBlock<T> t2;                         // [slabs][cols]: exp(-2 pi i (slab a) k / bins)
    DeviceBlock<int32_t> kcell;                // [cols]: LDS cell of each image column's bin (ro_band_windows.h)
    DeviceBlock<T> part;                       // [rows of a chunk][slabs][cols]
    size_t part_bytes = 0;
};

}  // namespace host
}  // namespace ro

struct ro_stft {
    template <typename T> using DeviceBlock = ro::host::DeviceBlock<T>;
    template <typename T> using PinnedBlock = ro::host::PinnedBlock<T>;

    ro_stft_config_t cfg{};
    int bins = 0, overlap = 0, hop = 0;
    int device = 0;
    std::string device_name;
    std::vector<float> window;
    DeviceBlock<float> d_window;
    DeviceBlock<float> d_window_k;     // kernel-order copy (single-pass plans)
    DeviceBlock<float> d_window_k32;   // ... in the order of the N = 32768 magnitude-row kernel (bins = 32768)
    DeviceBlock<float2> d_twiddles;
    DeviceBlock<float4> d_twiddles_k;  // packed copy for the radix-16/32 stages
    hipStream_t stream = nullptr;
    // extra band sets (ro_stft_set_extra_bands): scanned by ro_scan_sets.hip behind the primary's scan
    ro_bands_t extra[RO_MAX_EXTRA_BANDS] = {};
    int        extra_count = 0;
    // tile windows of the streaming path (ro_stft_set_tile_windows): cut by ro_cut_windows.hip behind each batch's rows
    ro_band_window_t tile_win[RO_MAX_TILE_WINDOWS] = {};
    int        tile_win_count = 0, tile_win_total = 0;

    // streaming state. Three HIP streams and RO_STREAM_SLOTS slots of device buffers: while the kernels of batch n run on
    // `stream`, batch n+1 is uploaded on `s_in` and batch n-1 goes home on `s_out`.
    int batch_rows = 0;
    // Samples are staged where the upload reads them: in the pinned buffer (h_in) of the slot the next batch will use
    // (slot = batch_seq % RO_STREAM_SLOTS), from its first byte.  A batch uploads the front of it and the samples later rows still
    // need -- the overlap and whatever came in behind the batch's last row -- are carried over to the other slot.
    int stage_fmt = RO_IQ_F32;                 // what is staged: RO_IQ_F32 (8 B per sample) or RO_IQ_I16 (4 B)
    bool stage_fmt_set = false;
    size_t  staged_have = 0;                   // live samples at the front of slot[batch_seq % RO_STREAM_SLOTS].h_in
    int64_t stream_sample0 = 0;                // stream index of the first of them
    // row sink (ro_stft_set_row_sink): finished rows go straight into the caller's ring (ro_pinned_alloc memory)
    float  *sink = nullptr;
    int64_t sink_stride = 0, sink_cap = 0, sink_first = 0;
    struct Slot {
        DeviceBlock<char> d_iq;                // batch input, bytes ((batch_rows-1)*hop + bins samples, 8 or 16 B each)
        DeviceBlock<float> d_rows;             // batch output (batch_rows x bins)
        DeviceBlock<float> d_tile;             // batch_rows x tile_cols when a tile is configured
        DeviceBlock<float> d_ln;               // ... its log and the rows' min / max of it (tile_ln)
        DeviceBlock<float> d_minmax;
        DeviceBlock<ro_scan_record_t> d_records;
        DeviceBlock<ro_scan_record_t> d_extra; // batch_rows x extra_count: the extra band sets' records
        DeviceBlock<float> d_image;            // batch_rows x tile_win_total: the tile windows' image
        PinnedBlock<char> h_in;                // pinned upload staging, bytes
        hipEvent_t uploaded = nullptr;         // H2D of this slot done (h_in reusable, kernels may start)
        hipEvent_t staging_free = nullptr;     // what the host waits for before it writes h_in again: `uploaded`, or the `done`
                                               // event of the graphed batch that last used the slot (not owned)
        hipEvent_t computed = nullptr;         // kernels of this slot done (d_iq reusable, D2H may start)
        hipEvent_t drained = nullptr;          // D2H of this slot done (d_rows / d_tile / d_records reusable)
        // latency-bound batches with a row sink (run_stream_batch): upload + kernels of a FULL batch of this slot as one
        // graph on the slot's own stream, captured from the very calls the plain path makes
        hipStream_t    gstream = nullptr;
        hipGraphExec_t gexec = nullptr;
        int            graph_fmt = -1;         // stage format the graph was captured for
        int64_t        uses = 0;               // batches this slot has run (the first one warms every lazy initialisation)
        bool           on_gstream = false;     // the slot's last batch ran on gstream (else on the three chained streams)
    } slot[RO_STREAM_SLOTS];
    bool slots_ready = false;
    hipStream_t s_in = nullptr, s_out = nullptr;
    bool graph_refused = false;                // stream capture of a batch failed once on this runtime: plain path only
    int out_first = 0, out_cols = 0;           // columns of every row that travel to the host (the tile, or all)
    int64_t batch_seq = 0;
    std::vector<ro::host::Batch *> batch_pool;           // recycled pinned batches
    int64_t rows_emitted = 0;                  // stream index of the next row to compute
    std::deque<ro::host::Batch *> ready;
    int64_t rows_ready = 0;
    int64_t stat_samples = 0, stat_rows = 0, stat_launches = 0;
    double stat_kernel_ms = 0.0;
    // per-call counters in the spirit of FFTBackend's RunningAverage2 trio (src/FFTBackend.h:86-92, :208-235)
    ro_stft_timing_t timing{};
    double push_ms_sum = 0.0, batch_ms_sum = 0.0, fetch_ms_sum = 0.0;
    int64_t timed_batches = 0, timed_rows = 0; // the batches behind batch_ms_sum (graphed batches are timed one in RO_GRAPH_TIME_EVERY)
    double  last_batch_ms = 0.0;               // ... and the last one's time, the estimate for the ones in between
    int64_t graph_batches = 0;
    int     diag_time_every = 0, diag_done_only = 0, diag_direct = 0;   // (-DRO_DIAG: tools/r5/host_calls_ab.py)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    DeviceBlock<unsigned long long> d_stamps;  // diagnostic builds (RO_STAMPS) only

    DeviceBlock<unsigned> d_ln_keys;   // 16 pairs of min / max keys of ro_stft_ln_tile_resident, used in turn
    unsigned ln_calls = 0;
    // large transforms (bins > 32768 = dec x sub_bins, decimation in frequency on the N = 32768 plan; see ro_stft_create)
    bool    big = false;
    int     sub_bins = 0, dec = 0;
    DeviceBlock<float2> d_tw_combine;  // [dec][sub_bins]: the rotations exp(-2 pi i q m / bins)
    bool    dif = false;               // 65536, 131072: one kernel sums the row's blocks itself (MODE 3)
    DeviceBlock<float>  d_window_dif;  // ... [dec][sub_bins]: window block r in the sub-plan's kernel order
    DeviceBlock<float2> d_dif_tw;      // ... exp(-2 pi i j / dec)
    DeviceBlock<float2> d_dif_shift;   // ... [dec][16]: the bin shift q / dec as the stages' twiddles (StftArgs::dif_shift)
    DeviceBlock<float2> d_spec;        // ... the folded sub-rows, [spec_rows][dec][sub_bins] float2
    DeviceBlock<float>  d_ones;        // ... a window of ones (the fold has applied the real one)
    int64_t spec_rows = 0;
    DeviceBlock<float2> d_spec2;       // complex spectra of a large size: the sub-rows' spectra before they are interleaved
    // bins = 262144, 524288: the magnitude rows as a four-step FFT (ro_fourstep.hip): column kernel, scratch, row kernel
    bool    four = false;
    DeviceBlock<float>  d_four_window; // the window in the column kernel's order
    DeviceBlock<float2> d_four_tw_a, d_four_tw_b, d_four_tw_r;                         // ro::FourArgs
    DeviceBlock<float>  d_four_z;      // [four_rows][bins] complex
    int64_t four_rows = 0;
    // lengths that are not a power of two (even 258 .. 524286): Bluestein's chirp-z form on an inner handle of the
    // power-of-two length czt_m >= 2 bins - 1 (see ro::CztArgs)
    bool    czt = false;
    int     czt_m = 0;
    ro_stft *inner = nullptr;
    DeviceBlock<float2> d_cw;          // [bins] window[i] * exp(-pi i i^2 / bins)
    DeviceBlock<float2> d_bc;          // [czt_m] conj(FFT_M(conj(chirp), wrapped)) / czt_m
    DeviceBlock<float2> d_czt_a, d_czt_A;              // [czt_rows][czt_m] each
    DeviceBlock<float>  d_czt_mag;                     // [czt_rows][czt_m]
    int64_t czt_rows = 0;

    // tile_ln: partial min / max of the fused epilogue's two tile waves (rows x 4 floats), grown on demand
    DeviceBlock<float> d_ln_part;
    int64_t ln_part_rows = 0;

    // the detector (ro_stft_events_resident): heads, tile totals and tile prefixes of one chunk (ro_events.h), allocated at
    // their full size (ro::EVENTS_SCRATCH_BYTES, under 0.5 MiB) by the first call -- the block never grows, so no launch
    // ever has to be waited for
    DeviceBlock<char> d_events_scratch;
    // the plan-then-copy calls' scratch, each grown by grow_scratch to what a call asks for.  Event snapshots
    // (ro_stft_snapshots_resident): the plan and the compacted pending lists of one call (ro_snapshots.h); grows with capacity
    // + pending_capacity
    DeviceBlock<char> d_snap_scratch;
    // raw I/Q of the events (ro_stft_raw_resident): the plan of one call (ro_raw.h); grows with pending_capacity +
    // dir_capacity
    DeviceBlock<char> d_raw_scratch;
    // FITS data units (ro_stft_snapshot_units_resident, ro_stft_raw_units_resident): the plan of one call (ro_units.h);
    // grows with dir_capacity; one block for each of the two calls (ro::UNITS_OF_IMAGES, ro::UNITS_OF_RAW), so that they do
    // not share a plan
    DeviceBlock<char> d_units_scratch[2];
    // grey-level previews: the plan and the blocks' keys of ro_stft_snapshot_levels_resident (ro_levels.h; grows with
    // dir_capacity and with the blocks levels_bytes holds), and the blocks' keys of ro_stft_periodic_levels_resident (grows
    // with the blocks of a plan); a block for each call, so that the two of a chunk do not share one
    DeviceBlock<char> d_levels_scratch[2];
    // preview files (ro_stft_levels_png_resident): the plan and the stored blocks' checksum parts of one call (ro_png.h);
    // grows with dir_capacity and with png_bytes
    DeviceBlock<char> d_png_scratch;
    // compressed preview files (ro_stft_levels_png_deflate_resident): the plan, every block's size, code table and checksum
    // parts of one call (ro_png_deflate.h); grows with dir_capacity and with levels_bytes
    DeviceBlock<char> d_png_deflate_scratch;
    // resized previews (ro_stft_levels_resize_resident): the intermediate images between the two passes of one call
    // (ro_resize.h); grows with the plan's mid_bytes
    DeviceBlock<char> d_resize_scratch;
    int cus = 0;                               // the device's compute units (device_cus; 0: not asked for yet)

    // band-only transform (ro_stft_band_resident, ro_stft_band_windows_resident): band_key is the window list the tables
    // belong to (one window for the consecutive call; empty: none); a handle has one precision, so one of the two sets is
    // in use (band64: RO_PRECISION_F64 handles of 131072 bins and above)
    std::vector<ro_band_window_t> band_key;
    ro::host::BandState<float2>  band;
    ro::host::BandState<double2> band64;

    // strict precision (RO_PRECISION_F64): double twiddle table + two complex-double scratch blocks
    bool     f64 = false;
    DeviceBlock<double2> d_tw_f64;
    // ... bins 256 ... 65536: the row in a CU's registers, no scratch (ro_f64reg.hip); its window order and twiddle tables
    bool     f64reg = false;
    DeviceBlock<float>   d_f64r_window;
    DeviceBlock<double2> d_f64r_tw[4];
    DeviceBlock<double2> d_scratch_d[2];
    int64_t  scratch_rows_d = 0;
    // (diagnostic builds, RO_F64_FUSED=1: round 5's one-launch form of the through-HBM passes, ro_f64fused.hip:
    // 8 rings of f64_ring_rows rows, the launch's control block, and its give-up word mirrored into pinned host memory)
    DeviceBlock<double2>  d_f64_ring;
    DeviceBlock<unsigned> d_f64_ctl;
    PinnedBlock<unsigned> h_f64_err;
    int       f64_ring_rows = 0, f64_wgs_per_cu = 0;
};

namespace ro {
namespace host {

// ---- ro_abi_helpers.cpp
void build_window(int kind, int bins, float *w);
// tile windows: nullptr if the list is valid, else why not (*which: the offending window, -1: the list itself)
const char *tile_windows_fault(int bins, const ro_band_window_t *w, int count, int64_t *total, int *which);
// ... as a refusal (RO_ERR_INVALID, the message names the offending window) in the name of entry point `who`
int tile_windows_check(const char *who, int bins, const ro_band_window_t *w, int count, int64_t *total);
// the window list and the image of a cut; rows_in / rows / row_stride are filled in by launch_tile_and_scan
ro::CutArgs make_cut_args(const ro_band_window_t *w, int count, float *d_image, int64_t image_stride);

// ---- ro_stft_capi.cpp
ro::StftArgs make_stft_args(const ro_stft *h, const void *d_iq, int64_t first_row, int64_t rows, float *d_rows,
                            int64_t row_stride, float *d_tile = nullptr, ro_scan_record_t *d_records = nullptr,
                            float *d_ln = nullptr);
// window -> FFT -> |X| for rows [first_row, +rows): the single-pass kernel, or for bins > 32768
// the one-kernel or the scratch form (ro_stft_create), in chunks that fit the scratch blocks
// d_tile / d_records (either may be null): produced here too, by the transform's own epilogue where the plan fuses them
// (N = 32768), by tile_kernel / scan_kernel behind it otherwise
int launch_transform(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float *d_rows,
                     int64_t row_stride, hipStream_t s, float *d_tile = nullptr, ro_scan_record_t *d_records = nullptr,
                     float *d_ln = nullptr);
// d_ln / d_minmax: the tile's log and the rows' min / max of it (tile_ln); need d_tile
// d_extra: rows x extra_count records of the handle's extra band sets (null: nothing is launched for them)
// cut: tile windows to copy out of these rows behind everything else (make_cut_args; null: none)
int launch_tile_and_scan(ro_stft *h, const float *d_rows, int64_t row_stride, int64_t rows, float *d_tile,
                         ro_scan_record_t *d_records, hipStream_t s, float *d_ln = nullptr, float *d_minmax = nullptr,
                         ro_scan_record_t *d_extra = nullptr, const ro::CutArgs *cut = nullptr);
int check_bands(const ro_stft *h, const ro_bands_t &b);
int ensure_ln_part(ro_stft *h, int64_t rows);
// a scratch block of the handle for a plan-then-copy call (ro_snapshots.cpp, ro_raw.cpp, ro_units.cpp), at least `need`
// bytes; the handle's device is current.  A block that has to grow is replaced, and an earlier launch on any stream may
// still be using the old one: the device is waited for before it goes.  A stream whose capacities stay the same allocates
// once and never waits
int grow_scratch(DeviceBlock<char> &block, size_t need);
// the device's compute units, asked for once per handle: they size those calls' copy grids; the handle's device is current
int device_cus(ro_stft *h, int *cus);
// the prelude of a plan-then-copy call, in this order: the handle's device made current, its compute units, `block` grown to
// `need` bytes
int scratch_for(ro_stft *h, DeviceBlock<char> &block, size_t need, int *cus);
int launch_spectra_big(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float2 *d_out,
                       int64_t out_stride, hipStream_t s);

// ---- ro_snapshots.cpp
// what every call that takes a row ring asks of it (null: refused too), as a refusal in the name of `who`
int ring_check(const char *who, const ro_row_ring_t *ring);

// ---- ro_png.cpp
// what the preview files' calls ask of their arguments, as a refusal in the name of `who`; d: "d_" where the arrays are the
// device's; aligned: the device's files start at multiples of 16 bytes of an aligned buffer
int png_check(const char *who, const char *d, bool aligned, const ro_fits_unit_t *level_dir, int64_t dir_capacity,
              const ro_unit_summary_t *level_summary, const void *levels, int64_t levels_bytes, const ro_fits_unit_t *png_dir,
              const void *png, int64_t png_bytes, const ro_unit_summary_t *png_summary);
// the two resident calls' arguments as the kernels take them (ro::PngArgs but the scratch)
void png_fill_args(ro::PngArgs &a, const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                   const void *levels, int64_t levels_bytes, ro_fits_unit_t *png_dir, void *png, int64_t png_bytes,
                   ro_unit_summary_t *png_summary);

// ---- ro_png_deflate.cpp
// a deflate block on the host: its bytes in the stream in the shorter form, and where that is the Huffman form every
// symbol's length and its code as the stream takes it
struct DeflateCode {
    int64_t bytes;
    bool huffman;
    uint8_t length[ro::DEFLATE_SYMS];
    uint16_t reversed[ro::DEFLATE_SYMS];
};
DeflateCode deflate_code(const unsigned char *raw, int64_t len, bool last);
// `len` raw bytes as one block at `out`, in the form `code` has chosen, stored for a null one; the bytes written
int64_t deflate_write_block(const unsigned char *raw, int64_t len, bool last, const DeflateCode *code, unsigned char *out);

// ---- ro_units.cpp
// the argument names a refusal speaks of: the units' calls and the levels' calls (ro_levels.cpp) ask the same of them
struct UnitNames {
    const char *dir, *buf, *bytes, *summary;       // "unit_dir", "units", "units_bytes", "unit_summary"
};
// what the calls over an arena ask of their common arguments, as a refusal in the name of `who`; d: "d_" where the arrays
// are the device's (the argument names of the resident calls), "" on the host; raw: the directory is ro_raw_capture_t (no
// cols, no slot windows); aligned: the device's stores are 16 bytes wide
int units_check(const char *who, const char *d, const UnitNames &names, bool raw, bool aligned, const void *dir,
                int64_t dir_capacity, const void *summary, const float *arena, int64_t arena_floats, int32_t cols,
                const ro_band_window_t *slot_windows, const ro_fits_unit_t *unit_dir, const void *units, int64_t units_bytes,
                const ro_unit_summary_t *unit_summary);
// The walk of every host twin that packs a source directory into a buffer: ro_snapshot_units_host, ro_raw_units_host,
// ro_snapshot_levels_host, ro_levels_png_host and ro_levels_png_deflate_host.  want(d) says what source entry d asks for:
// its status (RO_UNIT_SKIPPED, RO_UNIT_INVALID, or RO_UNIT_WRITTEN for a writable one), and for a writable one its shape,
// its data bytes and its room, a multiple of the call's block or alignment: 2880 bytes per block of a unit, 720 per block
// of a level image, png_room(bytes) for a file.  An entry is placed when the rooms up to and including its own are at most
// buf_bytes; then emit(d, dst) writes its `bytes` bytes, before the next want, and the rest of its room is zeroed here.
// The device plans of the units and the levels count in blocks: first_b + blocks <= buf_bytes / block, with the quotient
// rounded down.  For integers that are not negative that is (first_b + blocks) block <= buf_bytes, the rule in bytes.
// A room is below 2^62 -- a unit's is four times floats that lie in real memory, a file's is below 2^32 -- and so is the sum
// of the at most 2^24 rooms of a directory over real memory: first + room does not overflow
struct WalkWant {
    int32_t status;
    int32_t naxis1;
    int64_t naxis2;
    int64_t bytes;
    int64_t room;
};
template <class Want, class Emit>
void pack_walk(int64_t n, Want want, Emit emit, ro_fits_unit_t *dir, void *buf, int64_t buf_bytes, ro_unit_summary_t *summary)
{
    ro_unit_summary_t sum{};
    sum.entries = n;
    int64_t first = 0;                           // rooms of every writable entry so far, fitting or not
    for (int64_t d = 0; d < n; ++d) {
        const WalkWant w = want(d);
        ro_fits_unit_t out{};
        out.status = w.status;
        if (w.status == RO_UNIT_SKIPPED) sum.skipped += 1;
        else if (w.status == RO_UNIT_INVALID) sum.invalid += 1;
        else {
            out.bytes = w.bytes;
            out.naxis2 = w.naxis2;
            out.naxis1 = w.naxis1;
            if (first + w.room <= buf_bytes) {
                out.offset = first;
                unsigned char *dst = static_cast<unsigned char *>(buf) + first;
                emit(d, dst);
                std::memset(dst + w.bytes, 0, (size_t)(w.room - w.bytes));
                sum.written += 1;
                sum.units_bytes = first + w.room;
            } else {
                out.status = RO_UNIT_NO_ROOM;
                sum.no_room += 1;
            }
            first += w.room;
        }
        dir[d] = out;
    }
    sum.needed_bytes = first;
    *summary = sum;
}
// what a unit's or a level image's entry asks of the walk: `elem` bytes per pixel in blocks of `block` bytes -- 4 and 2880
// for a unit, 1 and 720 for a level image: the same number of blocks
inline WalkWant walk_want(const ro::UnitWant &w, int64_t elem, int64_t block)
{
    if (w.status != RO_UNIT_WRITTEN) return WalkWant{w.status, 0, 0, 0, 0};
    return WalkWant{w.status, w.naxis1, w.naxis2, elem * (int64_t)w.naxis1 * w.naxis2, ro::unit_blocks(w.naxis1, w.naxis2) * block};
}
// the entries of a source directory: n = min(max(resolved, 0), dir_capacity)
inline int64_t entries_of(int64_t resolved, int64_t dir_capacity) { return std::min(std::max<int64_t>(resolved, 0), dir_capacity); }
// what source entry d of an image directory asks for
inline ro::UnitWant unit_want_snapshot(const ro_snapshot_t &e, int32_t cols, int64_t arena_floats, const ro_band_window_t *slot_windows)
{
    const bool slot_ok = e.slot >= 0 && e.slot < ro::UNIT_SLOTS;
    return ro::unit_want_image(e.status, e.slot, e.rows, e.offset, cols, arena_floats, slot_ok ? slot_windows[e.slot].first_col : 0,
                               slot_ok ? slot_windows[e.slot].cols : 0);
}
// the resident calls' arguments as the plan takes them (ro::UnitsArgs but the scratch)
void units_fill_args(ro::UnitsArgs &a, const void *dir, int64_t dir_capacity, const void *summary, const float *arena,
                     int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows, ro_fits_unit_t *unit_dir,
                     void *units, int64_t units_bytes, ro_unit_summary_t *unit_summary);

// ---- ro_periodic.cpp
// the argument names a refusal speaks of: "units", "units_bytes"; and what the room is to the directory's unit offsets:
// "" for the units themselves, for the levels that it holds a quarter of them
struct PeriodicNames {
    const char *buf, *bytes, *room;
};
// what the calls over a plan's directory ask of their common arguments, as a refusal in the name of `who`; d: "d_" for the
// resident calls' argument names.  The buffer holds `block`-byte blocks, one for each 2880-byte block of the plan's units
// (2880 for the units, 720 for the levels).  Fills a: the ring and the WRITTEN entries of each recorder as one run
int periodic_check(const char *who, const char *d, const PeriodicNames &names, int64_t block, bool aligned,
                   const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count, const ro_periodic_entry_t *dir,
                   int64_t entries, void *buf, int64_t buf_bytes, ro::PeriodicArgs *a);

// ---- ro_czt.cpp
int czt_length(int bins);                       // the inner power-of-two length of an even bins that is not one, else 0
int czt_setup(ro_stft *h);                      // the inner handle and the chirp tables of a handle with h->czt
int launch_transform_czt(ro_stft *h, const void *d_iq, int format, int64_t first_row, int64_t rows, float *d_rows,
                         int64_t row_stride, hipStream_t s);

// ---- ro_stream.cpp
void destroy_batch(Batch *b);
void free_stream_slots(ro_stft *h);

}  // namespace host
}  // namespace ro
