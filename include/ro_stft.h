/*
 * ro_stft.h -- C ABI of the MI355X-native STFT / waterfall / bolid-scan path.
 *
 * This is the drop-in boundary for radio-observer's hot path.  Each entry point
 * names the reference interface (file:line under the reference tree) it
 * replaces.  Plain C types only: pointers, sizes, PODs.  No exceptions cross
 * this boundary; every call returns RO_OK (0) or a negative RO_ERR_* code and
 * ro_last_error() gives the text (the reference's own convention is
 * log-and-return, src/FFTBackend.cpp:194, src/WAVStream.cpp:209-213).
 *
 * One handle = one stream = one HIP stream; a handle is not thread-safe, which
 * mirrors the reference's single-caller rule for Backend::process()
 * (src/WAVStream.cpp:115-123, src/JackFrontend.cpp:15-39).
 *
 * There is NO CPU fallback behind this ABI: without a gfx950 device every
 * compute entry point fails with RO_ERR_HIP.
 */
#ifndef RO_STFT_H
#define RO_STFT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RO_OK               0
#define RO_ERR_INVALID     (-1)   /* bad argument / shape mismatch                */
#define RO_ERR_UNSUPPORTED (-2)   /* e.g. bins not a supported power of two       */
#define RO_ERR_HIP         (-3)   /* HIP runtime error or no device               */
#define RO_ERR_NOMEM       (-4)
#define RO_ERR_STATE       (-5)   /* call not valid in the handle's current state */

#define RO_ABI_VERSION 5

/* window function; the reference hard-codes the 4-term Nuttall
 * (src/FFTBackend.cpp:165-184) and keeps Hann as dead code (:157-163). */
enum { RO_WINDOW_NUTTALL = 0, RO_WINDOW_HANN = 1, RO_WINDOW_CUSTOM = 2 };

/* sample formats accepted by push / resident runs.
 *  F32: interleaved float32 I,Q -- RawStream's wire format (src/RawStream.cpp:33,61-62)
 *  I16: interleaved int16 I,Q, un-normalised -- WAVStream (src/WAVStream.cpp:119-120)
 *  F64: {double real; double imag;} -- struct Complex (src/Backend.h:26-29).
 *       RO_PRECISION_F64 handles of 256 ... 65536 bins stage, upload and multiply
 *       the doubles themselves ((double)sample x (double)w, src/FFTBackend.cpp:
 *       229-232) and also take them device-resident; every other handle accepts
 *       them through ro_stft_push only and narrows them to float32 while staging
 *       (lossless for every frontend the reference has: int16 WAV, float32 raw /
 *       JACK).  ro_stft_band_resident takes them device-resident and un-narrowed
 *       on RO_PRECISION_F64 handles of 131072 ... 1048576 bins. */
enum { RO_IQ_F32 = 0, RO_IQ_I16 = 1, RO_IQ_F64 = 2 };

/* arithmetic of the transform.
 *  F32: float32 butterflies on float32 samples -- the fast path; rows within 1e-5 of the ROW MAXIMUM of the
 *       reference's double-precision rows (measured 1-3e-7), which is the norm-wise reading of "1e-5 relative".
 *  F64: the reference's own arithmetic type -- double window multiply, double transform, double sqrt, one
 *       narrowing to the float row (src/FFTBackend.cpp:117-120,229-236, src/WaterfallBackend.cpp:492-505).  Bins
 *       256 ... 65536 keep the complex-double row in a compute unit's registers (samples read once, row written
 *       once; below 4096 bins 2 ... 16 rows share a workgroup); 131072 ... 1048576 are passes through HBM scratch.  Rows within 1e-5 of the reference PER BIN
 *       (measured <= 1.2e-7: one float32 ulp, at 60 dB of dynamic range); about 2.1 times slower than F32 at 32768 bins
 *       (0.203 against 0.430 of the HBM peak: profiles/r06_bench_line_final.json).
 *       Complex spectra (ro_stft_spectra_resident) up to 65536 bins.
 *  (Value 2 was ABI 4's RO_PRECISION_F64_ONE_LAUNCH, an experiment that measured slower; ro_stft_create answers
 *  RO_ERR_UNSUPPORTED for it.) */
enum { RO_PRECISION_F32 = 0, RO_PRECISION_F64 = 1 };

/* bin ranges of BolidRecorder::start (src/BolidRecorder.cpp:84-102), in
 * fft-shifted row columns.
 * Both bands lie inside [0, bins); a detect band may touch column 0 or column bins.  average() then reads avg_bins
 * columns from low_detect + peak - avg_bins / 2, and that window can leave the row: columns outside [0, bins)
 * count as 0, and the sum is still divided by avg_bins (the reference reads out of bounds there, src/BolidRecorder.cpp
 * :126-132; tests/test_gpu_scan_edges.py pins this on every kernel that scans). */
typedef struct ro_bands {
    int32_t low_noise;     /* lowNoiseBin_      */
    int32_t noise_width;   /* noiseWidth_       */
    int32_t low_detect;    /* lowDetectBin_     */
    int32_t detect_width;  /* detectWidth_      */
    int32_t avg_bins;      /* averageBinRange_  */
} ro_bands_t;

/* what BolidRecorder::update computes per row before its state machine
 * (src/BolidRecorder.cpp:121-132): n = noise(), p = peak(), a = average(). */
typedef struct ro_scan_record {
    float   noise;
    int32_t peak;
    float   average;
} ro_scan_record_t;

/* Construction parameters = WaterfallBackend::make's config keys
 * (src/WaterfallBackend.cpp:620-646) plus device-side options. */
typedef struct ro_stft_config {
    uint32_t     struct_size;      /* sizeof(ro_stft_config_t), for ABI growth     */
    int32_t      bins;             /* "bins"     default 32768                      */
    int32_t      overlap;          /* "overlap"  default 0; clamped to [0,bins-1]   */
    int32_t      sample_rate;      /* StreamInfo::sampleRate, default 48000         */
    int32_t      window_kind;      /* RO_WINDOW_*                                   */
    const float *window_table;     /* RO_WINDOW_CUSTOM: bins floats (host)          */
    double       iq_gain;          /* "iq_gain": added to Q (src/FFTBackend.cpp:79) */
    int32_t      iq_phase_shift;   /* must be 0 (non-zero is UB in the reference)   */
    int32_t      device;           /* HIP device ordinal                            */
    int32_t      max_batch_rows;   /* streaming: rows per launch (0 = default)      */
    int32_t      enable_scan;      /* compute ro_scan_record_t per row              */
    ro_bands_t   bands;            /* used when enable_scan                         */
    int32_t      tile_first_col;   /* compact band tile [tile_first_col, +tile_cols)*/
    int32_t      tile_cols;        /* 0 = no tile                                   */
    int32_t      spare_cus_per_xcd;/* CUs per XCD the persistent STFT grid leaves    */
                                   /* free (0..16).  The N >= 16384 kernels fill a   */
                                   /* CU's registers, so nothing else runs beside    */
                                   /* them; 1 lets a concurrent kernel on another    */
                                   /* stream (an RCCL collective) make progress.     */
    int32_t      precision;        /* RO_PRECISION_* (ABI 2; a caller that passes the */
                                   /* ABI-1 struct_size gets RO_PRECISION_F32)        */
    int32_t      tile_ln;          /* 1: with the tile, also its natural log and the  */
                                   /* per-row min / max of that log (the offline      */
                                   /* viewer's FN_LOG and colour range, fits2png:46,  */
                                   /* :476-477) straight from the transform; needs    */
                                   /* tile_cols > 0                                   */
} ro_stft_config_t;

typedef struct ro_stft ro_stft_t;

/* ---- library ------------------------------------------------------------- */
int         ro_abi_version(void);
const char *ro_last_error(void);          /* thread-local text of the last failure */
int         ro_device_count(void);        /* <0 on HIP error                        */

/* ---- pure host helpers: FFTBackend's public arithmetic -------------------- */
/* FFTBackend::FFTBackend overlap clamp, src/FFTBackend.cpp:108-109 */
int     ro_clamp_overlap(int bins, int overlap);
/* fftSampleRate_, src/FFTBackend.cpp:150-151 */
float   ro_fft_sample_rate(int sample_rate, int bins, int overlap);
/* FFTBackend::frequencyToBin, src/FFTBackend.h:159-178 */
int     ro_frequency_to_bin(int bins, int sample_rate, float frequency);
/* FFTBackend::binToFrequency, src/FFTBackend.h:134-147 */
float   ro_bin_to_frequency(int bins, int sample_rate, int bin);
/* FFTBackend::timeToFFTSamples, src/FFTBackend.h:197-200 */
int     ro_time_to_fft_samples(double seconds, float fft_sample_rate);
/* rows produced by FFTBackend::process for a stream of `samples`, :211-257 */
int64_t ro_row_count(int64_t samples, int bins, int overlap);
/* window table as FFTBackend::startStream builds it, :156-186 */
int     ro_window_table(int kind, int bins, float *out);
/* ---- time-chunk sharding of one stream over `world` GPUs ------------------------
 * Rows are independent (row r needs samples [r*hop, r*hop+bins) only,
 * src/FFTBackend.cpp:211-257), so shard g takes the contiguous rows
 * [floor(g*R/world), floor((g+1)*R/world)) and the samples under them; neighbouring
 * shards overlap by the bins-hop samples of halo.  Pure host arithmetic, no device. */
int     ro_shard_rows(int64_t total_rows, int world, int rank, int64_t *first_row, int64_t *rows);
/* first sample and sample count shard [first_row, +rows) must hold (halo included; 0 samples for an empty shard) */
int     ro_shard_samples(int64_t first_row, int64_t rows, int bins, int overlap,
                         int64_t *first_sample, int64_t *samples);
/* rows every rank contributes to an equal-block all-gather: the largest shard */
int64_t ro_shard_max_rows(int64_t total_rows, int world);
/* Stitch the result of an equal-block all-gather (world blocks of ro_shard_max_rows rows of
 * row_bytes each, short shards zero-padded at their end) into total_rows consecutive rows --
 * the row order the FITS writer (src/WaterfallBackend.cpp:141-211) and BolidRecorder's state
 * machine (src/BolidRecorder.cpp:171-273) consume.  Host memory; `out` may not alias `gathered`. */
int     ro_stitch_rows(const void *gathered, int64_t total_rows, int world, size_t row_bytes, void *out);
/* The one exchange step of a multi-GPU run, for a host that owns an RCCL communicator (one process per GPU): the
 * all-gather that puts every shard's rows (band tile, ln tile or 12-byte scan records) on every rank, in the equal-block
 * layout ro_stitch_rows / ro_stitch_rows_device undo.
 *   nccl_comm   the host's ncclComm_t; librccl is dlopen'ed on first use (RO_ERR_UNSUPPORTED if the box has none)
 *   d_local     device, local_rows x row_bytes: this rank's rows (local_rows as ro_shard_rows gives for `rank`)
 *   d_staging   device, ro_shard_max_rows x row_bytes of scratch (the zero-padded send block)
 *   d_gathered  device, world x ro_shard_max_rows x row_bytes
 * Asynchronous on `stream` (copy into the staging block, then ncclAllGather as bytes). */
int     ro_allgather_rows(void *nccl_comm, const void *d_local, int64_t local_rows, int64_t total_rows, int world,
                          int rank, size_t row_bytes, void *d_staging, void *d_gathered, void *stream);
/* The all-gather as the DIRECT exchange SURVEY 5 / 8(e) asks for ("prefer a direct all-to-all-write pattern ... over a
 * single ring": xGMI is point to point, seven links per GPU): inside one ncclGroupStart / ncclGroupEnd every rank
 * ncclSend's its local_rows x row_bytes to each peer and ncclRecv's each peer's rows AT THEIR STITCHED PLACE in d_out
 * (total_rows x row_bytes, device, on every rank) -- no zero-padded staging block, no stitch afterwards; the band the
 * consumer writes (src/WaterfallBackend.cpp:174-205) is complete on every rank when the stream reaches this point.
 * Asynchronous on `stream`. */
int     ro_allgather_rows_direct(void *nccl_comm, const void *d_local, int64_t local_rows, int64_t total_rows, int world,
                                 int rank, size_t row_bytes, void *d_out, void *stream);
/* The schedule of that direct exchange, one step of it: in step k (1 .. world - 1) rank `rank` sends its own rows to
 * *to = (rank + k) mod world and receives the rows of *from = (rank - k) mod world, which are rows
 * [*recv_first_row, +*recv_rows) of the stitched result -- every ordered pair of ranks meets in exactly one step, and
 * in every step every rank sends once and receives once (each xGMI link pair is used once per step).  k = 0 is the
 * rank's own copy (to = from = rank).  ro_allgather_rows_direct, ro_gather_rows (root: every step's receive; the
 * others: the one step whose `to` is the root) and timeshard.gather_rows_direct all walk this one function.
 * Pure host arithmetic. */
int     ro_direct_schedule(int world, int rank, int64_t total_rows, int k, int *to, int *from,
                           int64_t *recv_first_row, int64_t *recv_rows);
/* The same exchange when only ONE rank consumes the rows -- the reference's FITS writer and detector are one process
 * (src/WaterfallBackend.cpp:141-211, src/BolidRecorder.cpp:171-273): every rank sends its local_rows x row_bytes
 * straight to `root` (ncclSend / ncclRecv in one group: world - 1 transfers over world - 1 different links), where
 * they land at their own place in d_out (total_rows x row_bytes, device; ignored on the other ranks).  No padding,
 * no stitch.  Asynchronous on `stream`. */
int     ro_gather_rows(void *nccl_comm, const void *d_local, int64_t local_rows, int64_t total_rows, int world,
                       int rank, int root, size_t row_bytes, void *d_out, void *stream);
/* ro_stitch_rows for device memory: world device-to-device copies on `stream` */
int     ro_stitch_rows_device(const void *d_gathered, int64_t total_rows, int world, size_t row_bytes, void *d_out,
                              void *stream);
/* 1 if `bins` has a kernel in this build: powers of two 256 .. 1048576 (one kernel up to
 * 131072; above, two kernels and one trip through HBM scratch that the handle allocates on first
 * use: 8 bytes per bin and row for up to 1 GiB / (8 bins) rows at a time), and every other EVEN
 * length 258 .. 524286 (FFTW takes any N, src/FFTBackend.cpp:120; src/BolidRecorder.h:35
 * suggests 32728) as a chirp-z transform on the power-of-two length M >= 2 bins - 1 (scratch:
 * 20 M bytes per row for up to 1 GiB / (8 M) rows at a time).  Odd lengths have no defined
 * result in the reference (src/WaterfallBackend.cpp:489-505 leaves the last column unwritten). */
int     ro_bins_supported(int bins);

/* ---- handle --------------------------------------------------------------- */
/* FFTBackend::FFTBackend + startStream (src/FFTBackend.cpp:103-127, :144-189)
 * + WaterfallBackend::startStream's buffer sizing (src/WaterfallBackend.cpp:573-594). */
int ro_stft_create(const ro_stft_config_t *cfg, ro_stft_t **out);
/* FFTBackend::~FFTBackend, src/FFTBackend.cpp:130-141 */
int ro_stft_destroy(ro_stft_t *h);
int ro_stft_get_window(const ro_stft_t *h, float *out /* bins floats, host */);
int ro_stft_hop(const ro_stft_t *h);
int ro_stft_bins(const ro_stft_t *h);
int ro_stft_device_name(const ro_stft_t *h, char *buf, size_t len);
int ro_stft_set_bands(ro_stft_t *h, const ro_bands_t *bands);

/* ---- several band sets per row: one record per detector -----------------------
 * WaterfallBackend keeps a vector of recorders and calls every one of them for every row (src/WaterfallBackend.cpp:534-536,
 * :563-567), and each BolidRecorder derives its own noise band, detect band and averaging range in start()
 * (src/BolidRecorder.cpp:84-104): several detectors on one stream, each watching another frequency window.  A handle
 * serves up to 8 of them in one pass: the band set of ro_stft_config_t::bands / ro_stft_set_bands (the PRIMARY, unchanged
 * in every respect) and up to RO_MAX_EXTRA_BANDS extra sets, scanned from the rows the transform has just written. */
#define RO_MAX_EXTRA_BANDS 7
/* 0 <= count <= 7; count = 0 removes them.  Needs a primary set (enable_scan), else RO_ERR_STATE.
 * Every set is checked like ro_stft_set_bands; the message names the offending set's index.
 * count outside 0..7 gives RO_ERR_INVALID.  Only on an idle stream (nothing staged, nothing waiting
 * to be fetched), else RO_ERR_STATE.  Changing the sets drops the slots' captured graphs. */
int ro_stft_set_extra_bands(ro_stft_t *h, const ro_bands_t *sets, int count);
int ro_stft_extra_bands(const ro_stft_t *h, ro_bands_t *sets_out /* may be NULL */);   /* returns count */

/* ---- resident path (benchmarks, multi-GPU shards) --------------------------
 * Replaces, for rows [first_row, first_row+rows) of a stream that is already in
 * HBM, the whole of FFTBackend::process's row loop (src/FFTBackend.cpp:211-257)
 * and WaterfallBackend::processFFT's magnitude/shift (src/WaterfallBackend.cpp:485-505).
 *   d_iq        device pointer to sample 0 of the stream, `format` F32 or I16 (F64 too on RO_PRECISION_F64 handles of
 *               256 ... 65536 bins; RO_ERR_UNSUPPORTED elsewhere)
 *   samples     number of complex samples addressable at d_iq
 *   d_rows      device, rows x row_stride floats (row_stride >= bins); required
 *   d_tile      device, rows x tile_cols floats (compact copy of columns
 *               [tile_first_col, +tile_cols) of d_rows), or NULL
 *   d_records   device, rows records, or NULL (needs enable_scan)
 *   stream      hipStream_t as void* (NULL = the default stream, with its usual ordering rules)
 * The call is asynchronous on `stream`.  One handle = one stream: the handle owns scratch that some paths use
 * (bins > 131072, chirp-z lengths, RO_PRECISION_F64 above 65536 bins, tile_ln), so two launches of ONE handle may only be in flight
 * together when they are ordered on one stream -- like FFTBackend::process, which one thread calls at a time
 * (src/JackFrontend.cpp:19-22 only logs a re-entry).  Use one handle per concurrent stream. */
int ro_stft_run_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                         int64_t first_row, int64_t rows,
                         float *d_rows, int64_t row_stride,
                         float *d_tile, ro_scan_record_t *d_records, void *stream);

/* ro_stft_run_resident plus d_extra: device, rows x count records, record of extra set s of row r at [r * count + s].
 * d_extra == NULL behaves exactly like ro_stft_run_resident.  d_extra != NULL with count == 0 gives RO_ERR_STATE. */
int ro_stft_run_resident_sets(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row, int64_t rows,
                              float *d_rows, int64_t row_stride, float *d_tile,
                              ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream);

/* ro_stft_run_resident plus the viewer's log image of the tile, produced by the transform itself (tile_ln = 1):
 *   d_ln_tile    device, rows x tile_cols floats: logf(pixel) of every tile pixel (-inf for a zero pixel)
 *   d_ln_minmax  device, rows x 2 floats: min and max of that row's log over its NON-ZERO pixels (+inf, -inf for a
 *                row without any) -- the image's colour range (fits2png:476-477) is the min / max over its rows,
 *                and ro_ln_levels turns log values into the viewer's grey levels once that range is known
 * d_ln_minmax may be NULL.  For bins = 32768 the log is taken in the transform's epilogue, on the magnitudes still in LDS;
 * for the other sizes by a small kernel over the tile. */
int ro_stft_run_resident_ln(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                            int64_t first_row, int64_t rows, float *d_rows, int64_t row_stride,
                            float *d_tile, float *d_ln_tile, float *d_ln_minmax,
                            ro_scan_record_t *d_records, void *stream);
/* The viewer's grey levels of log values given the image's range: level = (uint8)((ln - mn) / (mx - mn) * 255) in
 * float32 arithmetic, truncating; -inf (a zero pixel) and a flat image give 0 (fits2png:444-445, :495-497).  Host. */
int ro_ln_levels(const float *ln, int64_t count, float mn, float mx, uint8_t *levels_out);

/* The complex spectra themselves instead of their magnitudes: what fftw_execute leaves in out_
 * (src/FFTBackend.cpp:236) and hands to the protected hook FFTBackend::processFFT(const fftw_complex *data,
 * int size, DataInfo, int rawMark) (src/FFTBackend.h:104) -- bin k of row r at d_spectra[r * stride + k] as
 * {float re, float im}, unshifted (k = 0 is DC), unnormalised, after gain and window like the magnitude path.
 * Same kernels with a different last step; rows x stride x 8 bytes are written.  Every size the handle supports:
 * one kernel up to 32768 bins, fold + transform + interleave through the handle's scratch above (power-of-two bins:
 * RO_ERR_UNSUPPORTED for chirp-z lengths).  An RO_PRECISION_F64 handle of 256 ... 65536 bins hands out its double
 * transform, each component narrowed to float once (every bin within a float32 ulp of the reference's fftw_complex,
 * however far below the row's largest); RO_ERR_UNSUPPORTED above.  Asynchronous on `stream`; one launch in flight per
 * handle above 32768 bins in float32 (the scratch is the handle's). */
int ro_stft_spectra_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                             int64_t first_row, int64_t rows,
                             float *d_spectra /* rows x stride x {re, im} */, int64_t stride, void *stream);

/* BolidRecorder::noise/peak/average over rows already in HBM
 * (src/BolidRecorder.cpp:121-132, :313-347). */
int ro_stft_scan_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                          ro_scan_record_t *d_records, void *stream);

/* ro_stft_scan_resident for all sets: d_records (primary) may be NULL, d_extra is required */
int ro_stft_scan_sets_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                               ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream);

/* The offline viewer's transform of a band image, on rows already in HBM (fits2png:46 FN_LOG,
 * :444-445 default_color_fn, :476-477 min/max, :495-497 the uint8 store):
 *   ln    = logf(pixel), float32, over columns [first_col, first_col+cols) of `rows` rows
 *   min/max of ln over the NON-ZERO pixels of the whole image (the viewer drops zeros)
 *   level = (uint8)((ln - min) / (max - min) * 255), float32 arithmetic, truncating
 * Zero pixels give -inf in d_ln and level 0; an image with max == min gives level 0 everywhere.
 *   d_ln      device, rows x cols floats, or NULL
 *   d_u8      device, rows x cols bytes,  or NULL
 *   d_minmax  device, 2 floats {min, max}, or NULL
 * Asynchronous on `stream`. */
int ro_stft_ln_tile_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                             int first_col, int cols, float *d_ln, uint8_t *d_u8, float *d_minmax,
                             void *stream);

/* ---- band-only transform ----------------------------------------------------
 * Nobody downstream reads a row whole: the snapshot recorder keeps the columns low_freq ... hi_freq of each row
 * (src/WaterfallBackend.cpp:174-205) and BolidRecorder::update reads the noise band, the detect band and the
 * average's window around the peak (src/BolidRecorder.cpp:121-132).  These three calls serve exactly that. */
/* 1 if ro_stft_band_resident can produce `cols` columns of a `bins`-bin row: bins a power of two
 * 16384 ... 1048576, 1 <= cols <= 1024.  Pure host. */
int ro_stft_band_supported(int bins, int cols);

/* The same question for a handle of the given precision.  RO_PRECISION_F32: ro_stft_band_supported.  RO_PRECISION_F64
 * (the reference's own arithmetic, src/FFTBackend.cpp:229-236, src/WaterfallBackend.cpp:497-503): bins a power of two
 * 131072 ... 1048576, 1 <= cols <= 1024 -- up to 65536 bins an FP64 handle's full row comes from registers without
 * scratch, and the band call stays refused there.  Any other precision: 0.  Pure host. */
int ro_stft_band_supported_precision(int bins, int cols, int precision);

/* Smallest column range that holds everything the recorders read of a row: the noise band (noise(),
 * src/BolidRecorder.cpp:313-317), the detect band (peak(), :323-335) widened by what average() reads around any peak
 * (:126-132, :338-347: [low_detect - avg_bins/2, low_detect + detect_width - 1 - avg_bins/2 + avg_bins)), and, if
 * tile_cols > 0, the tile (the snapshot's column cut, src/WaterfallBackend.cpp:176,204).
 * RO_ERR_INVALID if that range leaves [0, bins).  Pure host.  ONE band set and ONE range: ro_bands_windows below
 * answers for several sets, and keeps apart what lies apart. */
int ro_bands_hull(const ro_bands_t *bands, int bins, int tile_first_col, int tile_cols,
                  int *first_col, int *cols);

/* Columns [first_col, first_col + cols) of rows [first_row, +rows), and nothing else: no full row is
 * computed or written (the columns the snapshot cut of src/WaterfallBackend.cpp:176,204 keeps, or the three reads of
 * BolidRecorder::update, src/BolidRecorder.cpp:121-132).  d_band: device, rows x band_stride floats (band_stride >=
 * cols; floats beyond cols in a row are not touched).  d_records (optional; needs enable_scan and the handle's bands,
 * with the average's margin, inside the band -- RO_ERR_INVALID otherwise): the same records
 * ro_stft_scan_resident gives on the full row.  RO_PRECISION_F32 handles: RO_IQ_F32 / RO_IQ_I16, the float32 bar of
 * the rows (within 1e-5 of the FULL row's maximum).  RO_PRECISION_F64 handles of 131072 ... 1048576 bins: the same
 * columns in the reference's arithmetic (double window multiply, double transform, double sqrt, narrowed once:
 * src/FFTBackend.cpp:229-236, src/WaterfallBackend.cpp:497-503), RO_IQ_F32 / RO_IQ_I16 / RO_IQ_F64 (un-narrowed),
 * every bin within one float32 ulp of the reference's; d_band stays float32.
 * RO_ERR_UNSUPPORTED for FP64 handles of up to 65536 bins, chirp-z lengths and shapes
 * ro_stft_band_supported_precision refuses.  Two launches on the same input give the same
 * bits.  Asynchronous on `stream`; uses handle scratch, so one launch of a handle in flight at a time. */
int ro_stft_band_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                          int64_t first_row, int64_t rows, int first_col, int cols,
                          float *d_band, int64_t band_stride,
                          ro_scan_record_t *d_records, void *stream);

/* ---- band-only transform over several column windows --------------------------
 * What the recorders read of a row is seldom one run of columns: the noise band and the detect band of one detector lie
 * apart (radio-observer.json: 409 and 436 columns whose hull, with the snapshot's 615, is 1365), and several detectors
 * (ro_stft_set_extra_bands) watch different frequencies.  A WINDOW is one run of columns [first_col, first_col + cols)
 * of the fft-shifted row; the calls below compute up to RO_MAX_BAND_WINDOWS of them in one pass, 1024 columns in all, and
 * nothing of the columns between them.  (In X[k] = sum_a W^(a k) Z_a[k mod M] nothing asks the wanted k to be
 * consecutive or their residues mod M to differ: two columns of one residue read the same value Z_a, each with its own
 * twiddles.  A column's bits depend on its bin, on M and on the slab size only -- not on which other columns are asked
 * for.)  Rate, float32, radio-observer.json's two windows at 32768 bins: 0.37 x the full rows with tile and records
 * (profiles/band_windows.txt) -- the call serves shapes ro_stft_band_resident refuses and hosts that cannot afford the
 * rows in HBM; it is not a faster way to the same records there. */
#define RO_MAX_BAND_WINDOWS 8
typedef struct ro_band_window {
    int32_t first_col;             /* first column of the fft-shifted row           */
    int32_t cols;                  /* >= 1                                          */
} ro_band_window_t;

/* 1 if the windows are valid and a kernel exists for them: 1 <= count <= RO_MAX_BAND_WINDOWS, every cols >= 1, every
 * window inside [0, bins), ascending and not overlapping (touching is allowed), at most 1024 columns in all, and bins /
 * precision as ro_stft_band_supported_precision asks for that total (the short transforms are the smallest of 256, 512,
 * 1024 points that is at least the total).  Pure host. */
int ro_stft_band_windows_supported(int bins, const ro_band_window_t *windows, int count, int precision);

/* The windows that hold what `set_count` band sets (1 ... 8: a primary and its extras) read of a row, and the tile if
 * tile_cols > 0.  Per set two intervals, the noise band and the detect band widened by the average's margin (the two
 * ro_bands_hull joins into one); intervals that overlap or touch are merged; while more than RO_MAX_BAND_WINDOWS remain,
 * the pair with the smallest gap is merged (the lower pair on a tie).  windows_out: RO_MAX_BAND_WINDOWS entries,
 * ascending; *count_out of them are written.  RO_ERR_INVALID if an interval leaves [0, bins).  The total is not judged
 * here: ask ro_stft_band_windows_supported.  Pure host. */
int ro_bands_windows(const ro_bands_t *sets, int set_count, int bins, int tile_first_col, int tile_cols,
                     ro_band_window_t *windows_out, int *count_out);

/* ro_stft_band_resident over `count` windows.  Image layout: window w occupies floats [off_w, off_w + cols_w) of each
 * band row, off_w the sum of the earlier windows' cols; band_stride >= the total, floats beyond the total in a row are
 * not touched.  With count = 1 the bits are ro_stft_band_resident's.
 * d_records (optional): the primary set's records.  d_extra (optional; RO_ERR_STATE without extra sets): the handle's
 * extra sets' records, set s of row r at [r * extra_count + s] as in ro_stft_run_resident_sets.  Each requested set's
 * noise band must lie inside one window and its detect band, average's margin included, inside one window (not
 * necessarily the same) -- RO_ERR_INVALID naming the set and the columns otherwise.  The records are those of the scan
 * kernels on the band image, the bands moved to image coordinates (- first_col_w + off_w); peak counts from low_detect.
 * Precisions, formats, refusals, rows == 0 and the sample count: as ro_stft_band_resident.  Asynchronous on `stream`;
 * uses handle scratch, so one launch of a handle in flight at a time. */
int ro_stft_band_windows_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                                  int64_t first_row, int64_t rows,
                                  const ro_band_window_t *windows, int count,
                                  float *d_band, int64_t band_stride,
                                  ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream);

/* ---- tile windows: up to 8 column windows cut from each FULL row ---------------
 * WaterfallBackend keeps a vector of recorders and every SnapshotRecorder / BolidRecorder cuts its own [leftBin,
 * rightBin) out of each row (src/WaterfallBackend.cpp:174-205, :368-374).  A handle's one tile (tile_first_col,
 * tile_cols) can only serve them with the hull of everything.  A TILE WINDOW is a run of columns [first_col, first_col +
 * cols) of the fft-shifted row (ro_band_window_t); the calls below copy up to RO_MAX_TILE_WINDOWS of them out of full rows
 * into the IMAGE ro_stft_band_windows_resident defines: window w occupies floats [off_w, off_w + cols_w) of each image
 * row, off_w the sum of the earlier windows' cols; floats past the total in a row are never touched.  The rows come from
 * the full-row transform, so there is no cap on the total other than bins (radio-observer.json's bolid event band alone
 * is 2048 columns), every size, precision and format of ro_stft_run_resident is served, and a host may choose between
 * this and the band call by shape: the layout is the same. */
#define RO_MAX_TILE_WINDOWS 8

/* 1 if ro_bins_supported(bins) (chirp-z lengths included), 1 <= count <= RO_MAX_TILE_WINDOWS, every cols >= 1, every
 * window inside [0, bins), ascending and not overlapping (touching is allowed); else 0.  Pure host. */
int ro_tile_windows_supported(int bins, const ro_band_window_t *windows, int count);

/* The tile windows of a host with several recorders (src/WaterfallBackend.cpp:174-205, :368-374: each recorder's
 * [leftBin, rightBin)).  ranges: 1 <= range_count <= 32 column ranges, any order, overlaps allowed.  Ranges that overlap
 * or touch are merged; while more than RO_MAX_TILE_WINDOWS remain, the pair with the smallest gap is merged (the lower
 * pair on a tie) -- ro_bands_windows' rule.  windows_out: RO_MAX_TILE_WINDOWS entries, ascending, *count_out of them
 * written; they pass ro_tile_windows_supported wherever bins does.  offsets_out (range_count entries, may be NULL):
 * offsets_out[i] is the image column where ranges[i].first_col sits, so recorder i reads image columns [offsets_out[i],
 * + ranges[i].cols).  RO_ERR_INVALID for a range that leaves [0, bins), for cols < 1, for a count out of range.
 * Pure host. */
int ro_merge_windows(const ro_band_window_t *ranges, int range_count, int bins,
                     ro_band_window_t *windows_out, int *count_out, int32_t *offsets_out);

/* The windows' columns of `rows` rows that are already in HBM (like ro_stft_scan_resident): d_rows, rows x row_stride
 * floats (row_stride >= bins); d_image, rows x image_stride floats (image_stride >= the windows' total).  The image
 * equals d_rows[:, columns] exactly; a plain copy, each wanted float read once and written once.  rows == 0 is RO_OK
 * and writes nothing.  RO_ERR_INVALID for null pointers, image_stride < total, and a window list
 * ro_tile_windows_supported refuses (the message names the offending window).  Asynchronous on `stream`. */
int ro_stft_cut_windows_resident(ro_stft_t *h, const float *d_rows, int64_t row_stride, int64_t rows,
                                 const ro_band_window_t *windows, int count,
                                 float *d_image, int64_t image_stride, void *stream);

/* ro_stft_run_resident_sets with d_tile = NULL, then ro_stft_cut_windows_resident of the same rows on the same stream:
 * the rows, d_records and d_extra are the bits ro_stft_run_resident_sets gives (the records are scanned on the full
 * row, in row coordinates -- not image coordinates as in ro_stft_band_windows_resident), the image is those rows'
 * columns.  Every handle ro_stft_run_resident works on: any plan, float32 and RO_PRECISION_F64, chirp-z lengths, the
 * chunked paths.  A handle's configured tile is simply not produced by this call.  d_records / d_extra may be NULL.
 * Refusals as ro_stft_run_resident_sets and ro_stft_cut_windows_resident.  Asynchronous on `stream`. */
int ro_stft_run_resident_windows(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                                 int64_t first_row, int64_t rows, float *d_rows, int64_t row_stride,
                                 const ro_band_window_t *windows, int count,
                                 float *d_image, int64_t image_stride,
                                 ro_scan_record_t *d_records, ro_scan_record_t *d_extra, void *stream);

/* ---- the detector: events from scan records ------------------------------------
 * What BolidRecorder::update does with a row's record once noise(), peak() and average() are known: the decision
 * (src/BolidRecorder.cpp:135) and the three-state machine behind it (:171-267).  With mark = row + 1 (buffer_->mark(),
 * unwrapped) the machine has a closed form:
 *   detect(r) = (double)average > (double)noise * 2.0 (:135; false for a NaN), G = max(2, jitter) (:196-201: duration_
 *   counts from 1 at the first quiet row and is compared AFTER its increment, so a burst never ends sooner than two rows
 *   behind its last detect row).  Detect rows whose gaps are at most G - 1 quiet rows form one GROUP (STATE_BOLID <->
 *   STATE_BOLID_ENDED, :185-200).  A group with first detect row r0 and last detect row `last` FIRES at row last + G
 *   (:201-264), with  start_row = r0 + 1 - advance  (nextSnapshot_.start = mark - advance_, :178; may be negative),
 *   length = 2 advance + (last - r0 + 1)  (:179, :189: the quiet rows inside the group count, :196), and noise, peak,
 *   magnitude = the record of row r0 (:174-176; peak is the column, peakFreq_ = binToFrequency(low_detect + peak)).
 * A group whose fire row has not been seen yet is the carried state. */
typedef struct ro_detector {
    int32_t advance;               /* advance_ in rows (src/BolidRecorder.cpp:100), >= 0 */
    int32_t jitter;                /* jitter_ in rows (:101), >= 0                        */
} ro_detector_t;

typedef struct ro_event {          /* 40 bytes: the METEOR DETECTED branch, src/BolidRecorder.cpp:201-264 */
    int64_t fire_row;              /* the row whose update() fired                        */
    int64_t start_row;             /* nextSnapshot_.start, :178                           */
    int64_t length;                /* nextSnapshot_.length, :179, :189                    */
    float   noise;                 /* noise_, :175                                        */
    int32_t peak;                  /* the peak column behind peakFreq_, :174              */
    float   magnitude;             /* magnitude_, :176                                    */
    int32_t reserved;              /* 0                                                   */
} ro_event_t;

typedef struct ro_detect_state {   /* 32 bytes; all zero = STATE_INIT (:108), and every state that is not open is all zero */
    int64_t first_detect_row;      /* r0 of the open group                                */
    int64_t last_detect_row;       /* its last detect row so far                          */
    float   noise;                 /* the record of row r0 (:174-176)                     */
    int32_t peak;
    float   magnitude;
    int32_t open;                  /* 1: STATE_BOLID or STATE_BOLID_ENDED                 */
} ro_detect_state_t;

typedef struct ro_detect_summary { /* 24 bytes, per call */
    int64_t events;                /* events fired in the call, also those beyond `capacity` */
    int64_t detect_rows;           /* rows with detect(r)                                 */
    int64_t marginal_rows;         /* rows with fabs((double)a / (2.0 * (double)n) - 1.0) <= 1e-5: a decision that a last
                                    * bit of the transform could turn (SURVEY 7's per-mode figure) */
} ro_detect_summary_t;

/* The machine on the host, for ONE set: records[i * record_stride] is the record of row first_row + i (record_stride 1
 * for a primary's array, 1 + ... for a column of a [row][set] array such as ro_stft_fetch_sets hands out), rows >= 0.
 * state: in / out, zero-filled by the caller once.  An open state whose group could no longer fire (last_detect_row + G <
 * first_row: rows were left out) is closed silently.  events (capacity entries, NULL with capacity = 0): filled in
 * ascending fire_row; events beyond capacity are counted in summary->events and not written.  summary and detect (rows
 * bytes of 0 / 1) may be NULL.  rows == 0 changes nothing but *summary, which becomes zeros.  RO_ERR_INVALID for null
 * records (rows > 0), det or state, record_stride < 1, a negative advance, jitter, rows or capacity, and events == NULL
 * with capacity > 0.  Pure host, no device. */
int ro_events_host(const ro_scan_record_t *records, int64_t record_stride, int64_t first_row, int64_t rows,
                   const ro_detector_t *det, ro_detect_state_t *state, ro_event_t *events, int64_t capacity,
                   ro_detect_summary_t *summary, uint8_t *detect);

/* The same machine on the device for every set of the handle at once (csrc/ro_events.hip: a scan, three plain launches per
 * RO_EVENTS_CHUNK_ROWS rows), bit for bit what ro_events_host gives per set.  SLOT 0 is the primary (d_records, rows
 * records), slots 1 + s the handle's extra sets (d_extra[r * count + s], as ro_stft_run_resident_sets writes them).  Either
 * pointer may be NULL, not both; a NULL pointer's slots are left untouched in every output.
 *   detectors   host, 1 + count entries
 *   d_state     device, 1 + count entries, in / out; zero-filled by the caller once
 *   d_events    device, [slot][capacity], ascending fire_row; NULL with capacity = 0
 *   d_summary   device, 1 + count entries, overwritten by every call; may be NULL
 *   d_detect    device, [row][1 + count] bytes of 0 / 1; may be NULL
 * rows == 0 is RO_OK and changes nothing but the summaries, which become zeros.  RO_ERR_INVALID for a null handle or
 * state, both record pointers null, a negative rows or capacity, d_events == NULL with capacity > 0, a negative advance or
 * jitter (the message names the set); RO_ERR_STATE for d_extra on a handle without extra sets.  Asynchronous on `stream`;
 * uses handle scratch (the tiles' totals), so one launch of a handle in flight at a time unless they share a stream. */
int ro_stft_events_resident(ro_stft_t *h, const ro_scan_record_t *d_records, const ro_scan_record_t *d_extra,
                            int64_t first_row, int64_t rows, const ro_detector_t *detectors,
                            ro_detect_state_t *d_state, ro_event_t *d_events, int64_t capacity,
                            ro_detect_summary_t *d_summary, uint8_t *d_detect, void *stream);

/* ro_stft_run_resident_sets, then ro_stft_events_resident on the records it has just written, on the same stream: from
 * samples to events nothing waits for the host (src/FFTBackend.cpp:211-257 through src/BolidRecorder.cpp:119-267).  The
 * rows and records are the bits ro_stft_run_resident_sets gives; d_records, d_extra or both.  Every refusal of either call
 * is made before anything is launched. */
int ro_stft_run_resident_events(ro_stft_t *h, const void *d_iq, int format, int64_t samples, int64_t first_row, int64_t rows,
                                float *d_rows, int64_t row_stride, float *d_tile,
                                ro_scan_record_t *d_records, ro_scan_record_t *d_extra,
                                const ro_detector_t *detectors, ro_detect_state_t *d_state, ro_event_t *d_events,
                                int64_t capacity, ro_detect_summary_t *d_summary, uint8_t *d_detect, void *stream);

/* ---- event snapshots: each event's rows, cut from a row ring ---------------------
 * What the METEOR DETECTED branch ends in (src/BolidRecorder.cpp:262-263): startWriting() clamps the snapshot to
 * snapshotRows_ and reserves rows [start, start + length) of the row ring (src/WaterfallBackend.cpp:107-127); the worker
 * writes them once the ring holds them all (:60-104, :202-205).  A snapshot ends `advance` rows behind its group's last
 * detect row, so at the fire row it is routinely still incomplete.  Here the ring lives in HBM (the reference's
 * RingBuffer2D without its reservation: the caller sizes the ring instead), and one call per chunk reads the events where
 * ro_stft_events_resident left them, carries the incomplete ones from call to call and packs the rows of every complete
 * one into an arena with a directory.  The rows are opaque, `cols` floats each: the image of
 * ro_stft_run_resident_windows or ro_stft_band_windows_resident, a tile, or full rows. */
typedef struct ro_row_ring {       /* 32 bytes; the caller owns the memory */
    float   *d_rows;               /* device: ring_rows x stride floats; stream row r >= 0 lives in slot r % ring_rows */
    int64_t  stride;               /* floats between slots, >= cols; floats [cols, stride) of a slot are never touched */
    int64_t  ring_rows;            /* >= 1 */
    int32_t  cols;                 /* >= 1 */
    int32_t  reserved;             /* 0 */
} ro_row_ring_t;

enum { RO_SNAP_CAPTURED = 0, RO_SNAP_EMPTY = 1, RO_SNAP_LOST = 2 };

typedef struct ro_snapshot {       /* 72 bytes: one resolved event */
    ro_event_t event;              /* as ro_stft_events_resident wrote it */
    int64_t    first_row;          /* lo, below */
    int64_t    offset;             /* floats into d_arena: rows x cols floats, row-major, stride cols; 0 unless CAPTURED */
    int32_t    rows;               /* hi - lo if CAPTURED, else 0 */
    int32_t    slot;
    int32_t    status;             /* RO_SNAP_* */
    int32_t    reserved;           /* 0 */
} ro_snapshot_t;

typedef struct ro_snap_summary {   /* 64 bytes, one per call, overwritten by every call */
    int64_t resolved;              /* entries written to d_dir */
    int64_t captured, empty, lost; /* of those, by status */
    int64_t pending;               /* entries in the pending lists after the call, all slots of the mask */
    int64_t pending_dropped;       /* candidates that found no room in a pending list: gone, counted here */
    int64_t unlisted;              /* sum over the mask's slots of max(0, summary.events - capacity): fired but never written */
    int64_t arena_floats;          /* floats of d_arena used */
} ro_snap_summary_t;

/* Rows into the ring: row i of d_image (rows x image_stride floats, image_stride >= cols) is stream row first_row + i, and
 * its first `cols` floats go to slot (first_row + i) % ring_rows.  One launch; the wrap is computed in the kernel.  With
 * rows > ring_rows only the last ring_rows rows are written, so that every slot is stored exactly once and two runs give
 * the same bytes.  rows == 0 is RO_OK.  RO_ERR_INVALID for a null handle, ring, ring->d_rows or d_image, a negative
 * first_row or rows, image_stride < cols, and a ring with ring_rows < 1, cols < 1, stride < cols or reserved != 0.
 * Asynchronous on `stream`. */
int ro_stft_ring_put_resident(ro_stft_t *h, const float *d_image, int64_t image_stride, int64_t first_row, int64_t rows,
                              const ro_row_ring_t *ring, void *stream);

/* The snapshots of one call.
 *   d_events, capacity, d_summary   [slot][capacity] and [slot], exactly as ro_stft_events_resident leaves them; the number
 *                    of events of a slot is read ON THE DEVICE: min(d_summary[slot].events, capacity).  d_summary may be
 *                    NULL with capacity = 0 (no event is read, `unlisted` is 0)
 *   slot_mask        bit s: slot s takes part; the other slots are not read and not written anywhere (ro_stft_events_resident
 *                    leaves a NULL record pointer's slots untouched).  `slots` is the highest set bit plus one
 *   snapshot_rows    host, `slots` entries, each >= 1 where the mask has its bit: snapshotRows_
 *   ring, head_row   the caller states that stream rows [max(0, head_row - ring_rows), head_row) are in the ring: put
 *                    earlier on the same stream
 *   d_pending, d_pending_count   [slots][pending_capacity] events and [slots] counts, in / out, zero-filled by the caller
 *                    once (a count outside [0, pending_capacity] is read as the nearer bound); d_pending may be NULL with
 *                    pending_capacity = 0
 *   d_dir            room for slots x (capacity + pending_capacity) entries, so the directory cannot overflow
 *   d_arena          arena_floats floats; NULL with arena_floats = 0
 *   d_snap_summary   one entry
 * A slot's CANDIDATES are its pending list, in order, followed by this call's events, in order; slots in ascending order.
 * For a candidate e of slot s:  len = min(e.length, snapshot_rows[s])  (src/WaterfallBackend.cpp:113-115: the first rows are
 * kept),  lo = max(e.start_row, 0),  hi = e.start_row + len,  and, in this order:
 *   1  hi > head_row                  still PENDING: not resolved
 *   2  hi <= lo                       resolves as RO_SNAP_EMPTY
 *   3  lo < head_row - ring_rows      resolves as RO_SNAP_LOST: rows have been overwritten; nothing is written, no partial
 *                                     image (the reference's reservation would have blocked the writer instead)
 *   4  otherwise                      CAPTURABLE with (hi - lo) x cols floats
 * `offset` is the exclusive prefix sum of those sizes over all capturable candidates in (slot, order) order.  A capturable
 * candidate with offset + size <= arena_floats resolves as RO_SNAP_CAPTURED and its rows are copied from their ring slots;
 * the others -- by the prefix rule the first one that does not fit and every capturable one behind it -- stay pending and
 * come back in the next call.  Resolved candidates fill d_dir densely in (slot, order) order.  The still-pending ones become
 * the slot's new pending list in order; those beyond pending_capacity are dropped and counted.  Arena floats past
 * arena_floats used, directory entries past `resolved` and pending entries past the new counts are not touched.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, ring (or ring->d_rows),
 * snapshot_rows, d_pending_count, d_pending (pending_capacity > 0), d_dir or d_snap_summary; d_events == NULL or d_summary ==
 * NULL with capacity > 0; d_arena == NULL with arena_floats > 0; a negative capacity, pending_capacity, arena_floats or
 * head_row; a ring as ro_stft_ring_put_resident refuses it; slot_mask 0 or with bits at or above 1 + RO_MAX_EXTRA_BANDS; a
 * snapshot_rows entry below 1; more than 2^24 candidates in all (the mask's slots x (capacity + pending_capacity)).
 * Two plain launches (csrc/ro_snapshots.hip: the plan, then the copy), no atomics: equal inputs give equal bytes.  Asynchronous on `stream`; uses
 * handle scratch (the plan; it grows, waiting for the device, when capacity + pending_capacity grow), so one launch of a
 * handle in flight at a time unless they share a stream.  ro_stft_run_resident_windows (or the band call),
 * ro_stft_ring_put_resident, ro_stft_events_resident and this call read nothing on the host: issue them back to back. */
int ro_stft_snapshots_resident(ro_stft_t *h, const ro_event_t *d_events, int64_t capacity,
                               const ro_detect_summary_t *d_summary, uint32_t slot_mask, const int32_t *snapshot_rows,
                               const ro_row_ring_t *ring, int64_t head_row,
                               ro_event_t *d_pending, int64_t *d_pending_count, int64_t pending_capacity,
                               ro_snapshot_t *d_dir, float *d_arena, int64_t arena_floats,
                               ro_snap_summary_t *d_snap_summary, void *stream);

/* The same machine over host memory, candidate by candidate: every pointer is host memory, ring->d_rows included; no
 * device.  For a host that holds its rows itself (the streaming path), and the yardstick of the device call: equal inputs
 * give equal bytes in every output.  Refusals as above, without the handle. */
int ro_snapshots_host(const ro_event_t *events, int64_t capacity, const ro_detect_summary_t *summary, uint32_t slot_mask,
                      const int32_t *snapshot_rows, const ro_row_ring_t *ring, int64_t head_row,
                      ro_event_t *pending, int64_t *pending_count, int64_t pending_capacity,
                      ro_snapshot_t *dir, float *arena, int64_t arena_floats, ro_snap_summary_t *snap_summary);

/* ---- raw I/Q of each event: cut from the resident samples --------------------------
 * The other half of what the METEOR DETECTED branch writes: it sets includeRawData (src/BolidRecorder.cpp:262), and the
 * worker writes the I/Q samples behind the image as a 2 x L float image (writeRaw(), src/WaterfallBackend.cpp:77-81,
 * :214-267).  One call per chunk reads the snapshot directory where ro_stft_snapshots_resident left it and cuts each
 * captured event's samples out of the sample buffers the transform read, as (float)re, (float)im pairs
 * (FFTBackend::floatToInt, src/FFTBackend.h:250-254: the sample as delivered, before the I/Q gain), into an arena with a
 * directory.  There is no sample ring: the caller names the buffers that still hold the samples. */
#define RO_MAX_IQ_SPANS 4
typedef struct ro_iq_span {        /* 32 bytes: stream samples [first_sample, first_sample + samples) lie at d_iq */
    const void *d_iq;              /* device (host memory for ro_raw_host), in `format`, aligned to 8 bytes (RO_IQ_I16: 4) */
    int64_t     first_sample;      /* >= 0: unwrapped index into the stream */
    int64_t     samples;           /* >= 1 */
    int32_t     format;            /* RO_IQ_F32, RO_IQ_I16 or RO_IQ_F64, on any handle */
    int32_t     reserved;          /* 0 */
} ro_iq_span_t;

typedef struct ro_raw_capture {    /* 72 bytes: one resolved candidate */
    ro_event_t event;              /* as the snapshot directory held it */
    int64_t    first_sample;       /* f, below */
    int64_t    samples;            /* L if CAPTURED, else 0 */
    int64_t    offset;             /* floats into d_arena: `samples` pairs re, im; 0 unless CAPTURED */
    int32_t    slot;
    int32_t    status;             /* RO_SNAP_CAPTURED / RO_SNAP_EMPTY / RO_SNAP_LOST */
} ro_raw_capture_t;

typedef struct ro_raw_summary {    /* 64 bytes, overwritten by every call */
    int64_t resolved;              /* entries written to d_raw_dir */
    int64_t captured, empty, lost; /* of those, by status */
    int64_t pending;               /* entries in the pending list after the call */
    int64_t pending_dropped;       /* candidates that found no room in it: gone, counted here */
    int64_t arena_floats;          /* floats of d_arena used */
    int64_t reserved;              /* 0 */
} ro_raw_summary_t;

/* The raw runs of one call.
 *   d_dir, dir_capacity, d_snap_summary   the directory and the summary of ro_stft_snapshots_resident, as it leaves them;
 *                    the number of entries is read ON THE DEVICE: min(d_snap_summary->resolved, dir_capacity), at least 0
 *   spans, span_count   HOST array of 1 ... RO_MAX_IQ_SPANS buffers that hold the stream's samples (it travels in the
 *                    kernel arguments).  first_sample and first_sample + samples both ascend strictly from span to span,
 *                    and each span begins at or before the end of the one in front: no gap, overlap allowed (the chunk
 *                    buffers of a resident run overlap by bins - hop samples).  A sample several spans hold is read from
 *                    the LAST one that holds it.  base_sample = spans[0].first_sample, head_sample = the end of the last
 *                    span.  A host that double-buffers its uploads passes its last two or three chunk buffers
 *   d_pending, d_pending_count   ONE list of pending_capacity ro_snapshot_t and one count, in / out, zero-filled by the
 *                    caller once (a count outside [0, pending_capacity] is read as the nearer bound); d_pending may be
 *                    NULL with pending_capacity = 0
 *   d_raw_dir        room for pending_capacity + dir_capacity entries, so it cannot overflow
 *   d_arena          arena_floats floats, aligned to 8 bytes; NULL with arena_floats = 0
 *   d_raw_summary    one entry
 * The CANDIDATES are the pending list, in order (every entry of it), followed by the directory's entries whose status is
 * RO_SNAP_CAPTURED, in order.  EMPTY and LOST directory entries have no image and get no raw run: skipped, not resolved.
 * For a candidate c, with hop = bins - overlap of the handle (the clamped overlap) and z = (overlap == 0):
 *   start = c.event.start_row,  len = c.rows + (c.first_row - start)   the clamped length, also when the image was clipped
 *                                                                      at row 0
 *   L = (int64)(((double)len / (double)R) * (double)sample_rate),  R = (int)ro_fft_sample_rate(...): one division, one
 *       multiplication, truncated toward zero -- the recorder's fftSamplesToRaw (src/WaterfallBackend.h:84-87,
 *       src/WaterfallBackend.cpp:29-32: the rate is truncated to an int)
 *   f = (start - z) * hop + 1 for start >= 1, else 0 -- fftMarkToRaw(start): the handle at `start` was stamped by row
 *       start - 1 with the raw mark one slot ahead (src/WaterfallBackend.cpp:507), read after the overlap memmove
 *       (src/FFTBackend.cpp:242,251); on a fresh stream nobody has stamped the handles at or below 0 (mark 0)
 * and, in this order:
 *   1  f + L > head_sample            still PENDING: not resolved (the reference would write stale ring contents; L
 *                                     exceeds len x hop by up to fft rate / R, so this is no corner case)
 *   2  L <= 0                         resolves as RO_SNAP_EMPTY
 *   3  f < base_sample                resolves as RO_SNAP_LOST: nothing is written
 *   4  otherwise                      CAPTURABLE with 2 L floats
 * `offset` is the exclusive prefix sum of those sizes over all capturable candidates in order.  A capturable candidate
 * with offset + 2 L <= arena_floats resolves as RO_SNAP_CAPTURED and its samples are converted into the arena: RO_IQ_F32 a
 * bit copy, RO_IQ_I16 (float) of each int16, RO_IQ_F64 (float) of each double, round to nearest even (a result that is a
 * float32 denormal is not pinned).  No gain.  The others -- the first that does not fit and every capturable one behind it
 * -- stay pending.  Resolved candidates fill d_raw_dir densely, in order; the still-pending ones become the new list, in
 * order, those beyond pending_capacity dropped and counted.  Arena floats past arena_floats used, directory entries past
 * `resolved` and pending entries past the new count are not touched; neither are the sample buffers and d_dir.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, d_snap_summary, spans,
 * d_pending_count, d_raw_dir or d_raw_summary; d_dir == NULL with dir_capacity > 0; d_pending == NULL with
 * pending_capacity > 0; d_arena == NULL with arena_floats > 0 (or misaligned); a negative dir_capacity, pending_capacity or
 * arena_floats; span_count outside 1 ... RO_MAX_IQ_SPANS; a span with d_iq NULL (or misaligned), first_sample < 0,
 * samples < 1, an unknown format or reserved != 0; spans out of order or with a gap; more than 2^24 candidates
 * (pending_capacity + dir_capacity).  RO_ERR_UNSUPPORTED when R is 0 (the reference divides by zero there).
 * Two plain launches (csrc/ro_raw.hip: the plan, then the copy), no atomics: equal inputs give equal bytes.  Asynchronous
 * on `stream`; uses handle scratch (the plan; it grows, waiting for the device, when pending_capacity + dir_capacity
 * grow).  Nothing is read on the host: a chunk is ro_stft_run_resident_windows, ro_stft_ring_put_resident,
 * ro_stft_events_resident, ro_stft_snapshots_resident and this call, issued back to back. */
int ro_stft_raw_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                         const ro_snap_summary_t *d_snap_summary, const ro_iq_span_t *spans, int span_count,
                         ro_snapshot_t *d_pending, int64_t *d_pending_count, int64_t pending_capacity,
                         ro_raw_capture_t *d_raw_dir, float *d_arena, int64_t arena_floats,
                         ro_raw_summary_t *d_raw_summary, void *stream);

/* The same machine over host memory, candidate by candidate: every pointer is host memory, the spans' d_iq included; no
 * handle, no device (bins >= 2, overlap and sample_rate as ro_fft_sample_rate takes them).  The yardstick of the device
 * call: equal inputs give equal bytes in every output.  Refusals as above, without the handle and the alignments. */
int ro_raw_host(int bins, int overlap, int sample_rate, const ro_snapshot_t *dir, int64_t dir_capacity,
                const ro_snap_summary_t *snap_summary, const ro_iq_span_t *spans, int span_count,
                ro_snapshot_t *pending, int64_t *pending_count, int64_t pending_capacity,
                ro_raw_capture_t *raw_dir, float *arena, int64_t arena_floats, ro_raw_summary_t *raw_summary);

/* ---- event files: FITS data units cut to each recorder's columns -------------------
 * What is left between the two arenas above and the files: the worker writes rightBin_ - leftBin_ columns of every row for
 * the ONE recorder that fired (src/WaterfallBackend.cpp:176-177, :202-205; the raw image is 2 x L, :235, :258-261), and
 * FITSWriter stores every float big-endian and pads the data unit with zeros to a multiple of 2880 bytes
 * (src/FITSWriter.cpp).  One call per arena reads the directory where ro_stft_snapshots_resident (ro_stft_raw_resident) left
 * it and packs, for every captured entry, the data unit of its file: cut to the slot's columns, every float's four bytes
 * reversed, zero-padded to the block.  A host downloads the units in use, writes a header and makes one fwrite per file.
 * Headers, names, times and [compress] stay host work. */
#define RO_FITS_BLOCK 2880                     /* bytes; 720 floats */
enum { RO_UNIT_WRITTEN = 0, RO_UNIT_SKIPPED = 1, RO_UNIT_NO_ROOM = 2, RO_UNIT_INVALID = 3 };

typedef struct ro_fits_unit {      /* 32 bytes; entry d belongs to entry d of the source directory */
    int64_t offset;                /* bytes into d_units, a multiple of 2880; 0 unless WRITTEN */
    int64_t bytes;                 /* 4 * naxis1 * naxis2: the data; the unit occupies this rounded up to 2880 */
    int64_t naxis2;                /* rows (images) or samples (raw) */
    int32_t naxis1;                /* the slot's window cols (images) or 2 (raw) */
    int32_t status;                /* RO_UNIT_* */
} ro_fits_unit_t;

typedef struct ro_unit_summary {   /* 64 bytes, overwritten by every call */
    int64_t entries, written, skipped, no_room, invalid;
    int64_t units_bytes;           /* end of the last WRITTEN unit */
    int64_t needed_bytes;          /* 2880 * the blocks of ALL writable entries: the room that holds everything */
    int64_t reserved;              /* 0 */
} ro_unit_summary_t;

/* The data units of one snapshot arena.
 *   d_dir, dir_capacity, d_snap_summary   the directory and the summary of ro_stft_snapshots_resident, as it leaves them;
 *                    the number of entries is read ON THE DEVICE: n = min(max(d_snap_summary->resolved, 0), dir_capacity)
 *   d_arena, arena_floats, cols   the arena that call filled, and the floats of one of its rows (the ring's cols); NULL
 *                    with arena_floats = 0
 *   slot_windows     HOST array of 1 + RO_MAX_EXTRA_BANDS entries (it travels in the kernel arguments): where slot s's
 *                    recorder's columns sit in the IMAGE -- first_col = ro_merge_windows' offsets_out[i], cols = ranges[i].cols
 *                    -- or cols = 0: this recorder's files are not wanted
 *   d_unit_dir       room for dir_capacity entries; entry d describes d_dir[d], for d < n; entries at or behind n are not
 *                    touched
 *   d_units, units_bytes   the units, aligned to 16 bytes; NULL with units_bytes = 0
 *   d_unit_summary   one entry
 * For entry d < n, in this order:
 *   1  status != RO_SNAP_CAPTURED      RO_UNIT_SKIPPED
 *   2  slot outside [0, 1 + RO_MAX_EXTRA_BANDS), rows < 1, offset < 0, or offset + rows x cols > arena_floats
 *                                      RO_UNIT_INVALID: not what the producing call writes; nothing of it is read from the arena
 *   3  the slot's window has cols == 0 RO_UNIT_SKIPPED
 *   4  otherwise                       WRITABLE: naxis1 = the window's cols, naxis2 = rows, bytes = 4 naxis1 naxis2,
 *                                      blocks = ceil(bytes / 2880)
 * `offset` is 2880 x the exclusive prefix sum of `blocks` over all writable entries in directory order, fitting or not (the
 * snapshots' prefix rule: nothing behind the first entry that does not fit can fit).  A writable entry with offset +
 * 2880 blocks <= units_bytes is RO_UNIT_WRITTEN, the others RO_UNIT_NO_ROOM: they carry naxis1, naxis2 and bytes, with offset
 * 0, so that the host can size a second call from them and from needed_bytes.  SKIPPED and INVALID entries are zero but for
 * the status.  A written unit: float i = r naxis1 + c is arena float offset + r cols + first_col + c with its four bytes
 * reversed -- a bit copy: NaN payloads, -0 and denormals survive -- and the bytes from `bytes` to the end of the last
 * block are zero.  Bytes of d_units past the summary's units_bytes are not touched.  Nothing is remembered and the sources
 * are not written: a call can be repeated with a larger d_units.  (The periodic SnapshotRecorder has a call of its own,
 * ro_stft_periodic_units_resident below, from the ring straight to the units.)  n == 0 is RO_OK with a zero summary.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, d_snap_summary, slot_windows,
 * d_unit_dir or d_unit_summary; d_dir == NULL with dir_capacity > 0; d_arena == NULL with arena_floats > 0; d_units == NULL
 * with units_bytes > 0; d_units not aligned to 16 bytes; a negative dir_capacity, arena_floats or units_bytes; dir_capacity >
 * 2^24; cols < 1; a slot window with first_col < 0, cols < 0 or first_col + cols > cols; [d_units, + units_bytes)
 * overlapping the arena.
 * Two plain launches (csrc/ro_units.hip: the plan, then the copy), no atomics: equal inputs give equal bytes.  Asynchronous
 * on `stream`; uses handle scratch (the plan; it grows, waiting for the device, when dir_capacity grows) -- this call and
 * ro_stft_raw_units_resident each have a block of their own, so the two of a chunk may run on different streams; two calls of
 * the SAME kind on one handle share theirs: one in flight at a time unless they share a stream.  Nothing is read
 * on the host: a chunk is ... ro_stft_snapshots_resident, ro_stft_raw_resident and the two calls here, issued back to back. */
int ro_stft_snapshot_units_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                    const ro_snap_summary_t *d_snap_summary, const float *d_arena, int64_t arena_floats,
                                    int32_t cols, const ro_band_window_t *slot_windows,
                                    ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                                    ro_unit_summary_t *d_unit_summary, void *stream);

/* The data units of one raw arena: the same with the directory and the summary of ro_stft_raw_resident.  An entry is
 * INVALID with samples < 1, offset < 0 or offset + 2 samples > arena_floats; there is no slot window: naxis1 = 2,
 * naxis2 = samples, and float i of the unit is arena float offset + i.  Refusals as above, without cols and slot_windows
 * (null d_raw_summary). */
int ro_stft_raw_units_resident(ro_stft_t *h, const ro_raw_capture_t *d_raw_dir, int64_t dir_capacity,
                               const ro_raw_summary_t *d_raw_summary, const float *d_arena, int64_t arena_floats,
                               ro_fits_unit_t *d_unit_dir, void *d_units, int64_t units_bytes,
                               ro_unit_summary_t *d_unit_summary, void *stream);

/* The same rules over host memory, entry by entry: every pointer is host memory; no handle, no device.  The yardstick of
 * the device calls: equal inputs give equal bytes in every output.  Refusals as above, without the handle and the alignment. */
int ro_snapshot_units_host(const ro_snapshot_t *dir, int64_t dir_capacity, const ro_snap_summary_t *snap_summary,
                           const float *arena, int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                           ro_fits_unit_t *unit_dir, void *units, int64_t units_bytes, ro_unit_summary_t *unit_summary);
int ro_raw_units_host(const ro_raw_capture_t *raw_dir, int64_t dir_capacity, const ro_raw_summary_t *raw_summary,
                      const float *arena, int64_t arena_floats,
                      ro_fits_unit_t *unit_dir, void *units, int64_t units_bytes, ro_unit_summary_t *unit_summary);

/* ---- periodic snapshots: FITS data units cut from the row ring ---------------------
 * The recorder that is always on: the "snapshot" SnapshotRecorder of both station configurations writes [leftBin, rightBin)
 * of EVERY row into a file each snapshot_length seconds (src/WaterfallBackend.cpp:415-427, :107-127, :141-211).  Its cadence
 * has a closed form, every size is known on the host, and so the plan is host arithmetic and ONE launch goes from the
 * ring's slots to the big-endian, padded data units: no packed image, no directory on the device.
 * With mark = row + 1 and S = snapshotRows_ >= 1: snapshot k >= 0 is rows [k S, (k + 1) S).  update() queues it when
 * size(start) >= snapshotRows_ + 2 (:417), that is at row (k + 1) S + 1; startWriting() clamps the length to S (:113-115) and
 * the next snapshot starts at its end (:122-123).  With head_row = H (rows [0, H) have been seen) snapshot k is DUE iff
 * (k + 1) S + 2 <= H.  stop() (:400-403, writeUnfinished_) queues one more: [k' S, min((k' + 1) S, H)) for the first k' that
 * is not due -- the `final` one.
 * Two deviations: a final snapshot WITHOUT rows makes no entry (the reference's RingBuffer2D::size returns the ring's
 * capacity for an empty range and would write S stale rows); and a snapshot whose rows the ring no longer holds is LOST,
 * where the reference's reservation would have blocked the writer (as for the event snapshots above). */
#define RO_MAX_PERIODIC 8
enum { RO_PERIODIC_WRITTEN = 0, RO_PERIODIC_LOST = 1, RO_PERIODIC_NO_ROOM = 2 };

typedef struct ro_periodic {       /* 12 bytes: one periodic recorder */
    int32_t          snapshot_rows;            /* S >= 1: ro_snapshot_rows */
    ro_band_window_t window;                   /* its [leftBin, rightBin) in RING columns: cols >= 1, inside the ring's cols */
} ro_periodic_t;

typedef struct ro_periodic_entry { /* 56 bytes: one snapshot of one recorder */
    int64_t index;                 /* k */
    int64_t first_row;             /* k S */
    int64_t due_row;               /* the row whose update() queues it: (k + 1) S + 1; H - 1 for the final one */
    int64_t offset;                /* bytes into the units, a multiple of 2880; 0 unless WRITTEN */
    int64_t bytes;                 /* 4 naxis1 rows: the data; the unit occupies this rounded up to 2880.  0 if LOST */
    int32_t rows;                  /* naxis2: S, or what the final one has, 1 ... S */
    int32_t naxis1;                /* the window's cols */
    int32_t recorder;
    int32_t status;                /* RO_PERIODIC_* */
} ro_periodic_entry_t;

typedef struct ro_periodic_summary {           /* 64 bytes, overwritten by every call */
    int64_t entries, written, lost, no_room;
    int64_t unlisted;              /* candidates beyond `capacity`: not listed, not advanced */
    int64_t units_bytes;           /* end of the last WRITTEN unit */
    int64_t needed_bytes;          /* 2880 * the blocks of ALL listed writable entries: the room that holds them */
    int64_t reserved;              /* 0 */
} ro_periodic_summary_t;

/* snapshotRows_ of a recorder: (int)ceil(snapshot_length * fft rate) with the float rate of ro_fft_sample_rate, at least 1
 * (SnapshotRecorder::requestBufferSize, src/WaterfallBackend.cpp:339-345; the ring it asks for is 8 times that). */
int ro_snapshot_rows(int sample_rate, int bins, int overlap, int snapshot_length);

/* The plan of one call: pure host arithmetic, no handle, no device.
 *   recorders, count   1 ... RO_MAX_PERIODIC recorders; windows in columns of a ring row of `cols` floats
 *   next_index         host, [count], in / out, zero-filled once: the first snapshot of each recorder that is not resolved
 *   head_row, final    H >= 0: rows [0, H) are in the stream, and the ring holds [max(0, H - ring_rows), H); final != 0: stop()
 *   ring_rows, cols    of the ring the units will be cut from
 *   units_bytes        room of the units buffer
 *   dir, capacity      room for `capacity` entries (NULL with 0); entries behind the summary's `entries` are not touched
 * A recorder's CANDIDATES are its due snapshots k = next_index, next_index + 1, ... and, with `final`, the final one if it
 * has rows (a next_index beyond the first snapshot that is not due says that the final one has resolved already: none);
 * recorders in ascending order.  For each, in this order:
 *   1  first_row < H - ring_rows      RO_PERIODIC_LOST: it resolves, nothing is written; it carries rows and naxis1
 *   2  otherwise                      WRITABLE with blocks = ceil(4 naxis1 rows / 2880)
 * `offset` is 2880 x the exclusive prefix sum of `blocks` over the writable candidates.  A writable candidate with offset +
 * 2880 blocks <= units_bytes is RO_PERIODIC_WRITTEN; the first that does not fit and every writable one behind it, of any
 * recorder, is RO_PERIODIC_NO_ROOM: it has its shape and offset 0, is not resolved and comes back in the next call.  A
 * recorder's next_index advances past its LEADING resolved entries only.  Candidates beyond `capacity` are not listed and
 * not advanced; the summary counts them.  Called with any sequence of non-decreasing head_row, repeats included, the plan
 * yields each snapshot exactly once in total.  The host knows due_row from here: the 12-byte scan record behind a
 * snapshot's listenToNoise_ CSV line (:157-167) is a copy the host issues itself.
 * RO_ERR_INVALID, the text naming the argument: null recorders, next_index or summary; dir == NULL with capacity > 0; count
 * outside 1 ... RO_MAX_PERIODIC; snapshot_rows < 1; a window with first_col < 0, cols < 1 or first_col + cols > cols; a
 * negative head_row, units_bytes, capacity or next_index entry (or rows beyond 2^62); ring_rows < 1; cols < 1. */
int ro_periodic_plan(const ro_periodic_t *recorders, int count, int64_t *next_index, int64_t head_row, int final,
                     int64_t ring_rows, int32_t cols, int64_t units_bytes,
                     ro_periodic_entry_t *dir, int64_t capacity, ro_periodic_summary_t *summary);

/* The units of one plan: ONE plain launch (csrc/ro_periodic.hip), ring -> units.  dir is HOST memory, as ro_periodic_plan
 * left it, `entries` of them; nothing but scalars reaches the kernel (per recorder its first written snapshot, how many, S,
 * the window, the blocks of a unit and where the first one starts: all in the kernel arguments).  No directory upload, no
 * plan kernel, no handle scratch.  A written unit: float i = r naxis1 + c is ring float
 * ((first_row + r) % ring_rows) stride + first_col + c with its four bytes reversed -- a bit copy -- and the bytes from
 * `bytes` to the end of the last block are zero.  The ring is only read; bytes of d_units behind the last written unit are
 * not touched; no atomics: equal inputs give equal bytes.  Asynchronous on `stream`: issue it behind
 * ro_stft_ring_put_resident on the same stream, with the head_row the plan was given in the ring.  entries == 0, or none
 * WRITTEN, launches nothing.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, ring, ring->d_rows, recorders or
 * dir (entries > 0); a ring as ro_stft_ring_put_resident refuses it; count outside 1 ... RO_MAX_PERIODIC; snapshot_rows <
 * 1; a window with first_col < 0, cols < 1 or first_col + cols > ring->cols; a negative entries or units_bytes; d_units ==
 * NULL with units_bytes > 0, or not aligned to 16 bytes; [d_units, + units_bytes) overlapping the ring; a directory that is
 * not what the plan writes for these recorders: recorders ascending, a recorder's indices consecutive, first_row = index x
 * S, rows = S but for a recorder's last entry (1 ... S), rows <= ring_rows, naxis1 and bytes those of the window, an
 * unknown status, a WRITTEN entry behind a NO_ROOM one, and the WRITTEN entries' offsets the multiples of 2880 that pack
 * them from 0 on, inside units_bytes.
 * The older route keeps working: un-wrap the ring into a packed image, build ro_snapshot_t entries by hand, then
 * ro_stft_snapshot_units_resident. */
int ro_stft_periodic_units_resident(ro_stft_t *h, const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                    const ro_periodic_entry_t *dir, int64_t entries, void *d_units, int64_t units_bytes,
                                    void *stream);

/* The same rules over host memory, ring->d_rows included: no handle, no device.  The yardstick of the device call: equal
 * inputs give equal bytes.  Refusals as above, without the handle and the alignment. */
int ro_periodic_units_host(const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                           const ro_periodic_entry_t *dir, int64_t entries, void *units, int64_t units_bytes);

/* ---- grey-level previews: each snapshot's ln image as uint8 -------------------------
 * What the stations make of every one of those files next: fits2png's natural log of the non-zero pixels, the image's own
 * min / max of it and (ln - min) / (max - min) * 255 as one byte per pixel (fits2png:46, :444-445, :476-502).  The two
 * calls here make that preview for every image of a snapshot directory and of a periodic plan, a quarter of the units'
 * bytes to download.
 * Geometry: a level image of naxis1 x naxis2 pixels occupies naxis1 naxis2 bytes, row-major with stride naxis1, the first
 * FFT row first, and is zero-padded to a multiple of RO_LEVEL_BLOCK bytes.  ceil(p / 720) = ceil(4 p / 2880): an image has
 * exactly as many 720-byte blocks as its FITS unit has 2880-byte ones, and packed the same way it sits at a quarter of its
 * unit's offset.  d_levels is aligned to 16 bytes, and so is every image (720 = 16 x 45).
 * Pixel rule, that of ro_stft_ln_tile_resident, bit for bit: l = logf(v) in float32; the range is the min / max of l over
 * the image's pixels with v != 0; level = (v != 0 && max > min) ? (uint8)(int)((l - min) / (max - min) * 255.f) : 0, all in
 * float32.  An image without a non-zero pixel has the range {+inf, -inf} and all levels 0.  Pixels that are NaN, +-inf or
 * negative are not pinned. */
#define RO_LEVEL_BLOCK 720                     /* bytes = pixels; RO_FITS_BLOCK / 4 */

typedef struct ro_level_range {    /* 8 bytes: the colour range of one image */
    float ln_min, ln_max;          /* min / max of logf over its non-zero pixels; +inf, -inf without one */
} ro_level_range_t;

/* The level images of one snapshot arena.  The arguments of ro_stft_snapshot_units_resident, with
 *   d_level_dir      room for dir_capacity entries, in LEVEL terms: offset is bytes into d_levels, a multiple of 720; bytes =
 *                    naxis1 naxis2.  With levels_bytes = units_bytes / 4 it is the unit directory with offset and bytes
 *                    divided by four.  Entries at or behind n are not touched
 *   d_ranges         room for dir_capacity entries (NULL with dir_capacity = 0): d_ranges[d] is entry d's range if it is
 *                    WRITTEN and {0, 0} otherwise, for d < n; entries at or behind n are not touched
 *   d_levels, levels_bytes   the images, aligned to 16 bytes; NULL with levels_bytes = 0
 *   d_level_summary  one entry; units_bytes and needed_bytes count level bytes (needed_bytes sizes a second call)
 * Entry rules 1 - 4 of ro_stft_snapshot_units_resident apply unchanged, in order; the entry count is read on the device; the
 * prefix rule is the same over 720-byte blocks with the room levels_bytes; the statuses are RO_UNIT_*; NO_ROOM entries carry
 * their shape with offset 0.  Bytes of d_levels past the summary's units_bytes are not touched; the sources are only read;
 * equal inputs give equal bytes.
 * Plain launches (csrc/ro_levels.hip), no atomics, no workgroup waiting for another: the units' plan; a reduce over the
 * 720-pixel blocks that leaves each block's min / max in handle scratch; a fold of each entry's blocks into d_ranges; the
 * store.  Asynchronous on `stream`; the scratch is this call's own (it grows, waiting for the device, with dir_capacity
 * and with the blocks levels_bytes holds): one call in flight per handle unless they share a stream.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: as ro_stft_snapshot_units_resident refuses
 * (d_level_dir, d_levels, levels_bytes and d_level_summary in the place of the units' arguments); d_ranges == NULL with
 * dir_capacity > 0; [d_levels, + levels_bytes) overlapping the arena; levels_bytes above 2^61. */
int ro_stft_snapshot_levels_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                     const ro_snap_summary_t *d_snap_summary, const float *d_arena, int64_t arena_floats,
                                     int32_t cols, const ro_band_window_t *slot_windows,
                                     ro_fits_unit_t *d_level_dir, ro_level_range_t *d_ranges, void *d_levels,
                                     int64_t levels_bytes, ro_unit_summary_t *d_level_summary, void *stream);

/* The level images of one periodic plan.  dir is HOST memory, exactly what ro_periodic_plan left for the units (the plan
 * cannot be asked twice: next_index advances), so the levels ride on the units' plan: the image of a WRITTEN entry e sits
 * at e.offset / 4 of d_levels, d_ranges[e] (device, `entries` of them) is written for WRITTEN entries and not touched for
 * the others, and levels_bytes must hold a quarter of the end of the last WRITTEN unit.  Only scalars reach the kernels:
 * three launches (reduce, fold, store), no plan kernel, no directory upload; handle scratch for the blocks' min / max (a
 * block of this call's own).  The ring is only read; bytes of d_levels behind the last written image are not touched; no
 * atomics: equal inputs give equal bytes.  Asynchronous on `stream`: issue it behind ro_stft_ring_put_resident, next to
 * ro_stft_periodic_units_resident.  entries == 0, or none WRITTEN, launches nothing.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: as ro_stft_periodic_units_resident refuses,
 * the directory's consistency included (d_levels and levels_bytes in the place of d_units and units_bytes; the WRITTEN
 * entries' units lie inside 4 x levels_bytes); d_ranges == NULL with a WRITTEN entry; d_levels not aligned to 16 bytes;
 * [d_levels, + levels_bytes) overlapping the ring. */
int ro_stft_periodic_levels_resident(ro_stft_t *h, const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                                     const ro_periodic_entry_t *dir, int64_t entries, ro_level_range_t *d_ranges,
                                     void *d_levels, int64_t levels_bytes, void *stream);

/* The same rules over host memory (ring->d_rows included): no handle, no device, the C library's logf and ro_ln_levels'
 * arithmetic.  Directories, summaries, offsets, padding and untouched bytes are those of the device calls; levels and
 * ranges differ by what the two logf differ.  Refusals as above, without the handle and the alignment. */
int ro_snapshot_levels_host(const ro_snapshot_t *dir, int64_t dir_capacity, const ro_snap_summary_t *snap_summary,
                            const float *arena, int64_t arena_floats, int32_t cols, const ro_band_window_t *slot_windows,
                            ro_fits_unit_t *level_dir, ro_level_range_t *ranges, void *levels, int64_t levels_bytes,
                            ro_unit_summary_t *level_summary);
int ro_periodic_levels_host(const ro_row_ring_t *ring, const ro_periodic_t *recorders, int count,
                            const ro_periodic_entry_t *dir, int64_t entries, ro_level_range_t *ranges, void *levels,
                            int64_t levels_bytes);

/* ---- preview files: each level image as a complete PNG ------------------------------
 * What a station publishes of a preview is a .png.  One call turns every level image of a level directory into the bytes
 * of that file: 8 bit, grey, no interlace; a filter byte 0 in front of every scanline; the zlib stream in STORED deflate
 * blocks (no compression here: ro_stft_levels_png_deflate_resident below Huffman-codes the blocks; LZ77 and filter choice
 * stay out of scope, and so do fits2png's legend and axes; its --width is ro_stft_levels_resize_resident); the Adler-32, the IDAT CRC-32, IEND.  A host downloads the files in use and makes one fwrite per file.
 * For an image of W = naxis1 by H = naxis2 pixels: R = H (W + 1) raw bytes, the first FFT row first, in nblk =
 * ceil(R / 65535) stored blocks, every one but the last of exactly 65535 bytes:
 *   89 50 4E 47 0D 0A 1A 0A                                   the signature, 8 bytes
 *   00 00 00 0D "IHDR" W(be32) H(be32) 08 00 00 00 00 crc     25 bytes
 *   len(be32) "IDAT"                                          len = 6 + 5 nblk + R
 *     78 01                                                   the zlib header
 *     nblk x { BFINAL (01 on the last, else 00), LEN (le16), ~LEN (le16), LEN raw bytes }
 *     adler32(be32) over the R raw bytes
 *   crc(be32) over "IDAT" and its data
 *   00 00 00 00 49 45 4E 44 AE 42 60 82                       IEND
 * 63 + 5 nblk + R bytes.  Block k's header sits at file byte 43 + 65540 k and its raw bytes at 48 + 65540 k.  An image
 * whose IDAT length would exceed 2^31 - 1 cannot be a PNG. */
#define RO_PNG_ALIGN 16                        /* bytes: where a file starts in the buffer */

/* The bytes of that file, or RO_ERR_INVALID for naxis1 < 1, naxis2 < 1 or an IDAT beyond 2^31 - 1.  Pure host. */
int64_t ro_png_bytes(int32_t naxis1, int64_t naxis2);

/* The files of one level directory.
 *   d_level_dir, dir_capacity, d_level_summary   the directory and the summary of ro_stft_snapshot_levels_resident, as it
 *                    leaves them (or the upload of what ro_periodic_level_dir makes of a periodic plan); the number of
 *                    entries is read ON THE DEVICE: n = min(max(d_level_summary->entries, 0), dir_capacity)
 *   d_levels, levels_bytes   the level images; NULL with levels_bytes = 0
 *   d_png_dir        room for dir_capacity entries; entry d describes d_level_dir[d], for d < n: offset is bytes into
 *                    d_png, a multiple of RO_PNG_ALIGN; bytes is the file's exact size; naxis1 and naxis2 are the image's.
 *                    Entries at or behind n are not touched
 *   d_png, png_bytes the files, aligned to 16 bytes; NULL with png_bytes = 0
 *   d_png_summary    one entry; units_bytes is the end of the last written file rounded up to 16, needed_bytes the room
 *                    that holds every writable one
 * For entry d < n, in this order:
 *   1  status != RO_UNIT_WRITTEN       RO_UNIT_SKIPPED
 *   2  naxis1 < 1, naxis2 < 1, bytes != naxis1 naxis2, offset < 0, offset not a multiple of RO_LEVEL_BLOCK, offset + bytes >
 *      levels_bytes, or a shape ro_png_bytes refuses
 *                                      RO_UNIT_INVALID: nothing of it is read from the levels
 *   3  otherwise                       WRITABLE: its file occupies ro_png_bytes rounded up to 16
 * `offset` is the exclusive prefix sum of those rounded sizes over all writable entries in directory order, fitting or not
 * (the family's prefix rule).  A writable entry with offset + its rounded size <= png_bytes is RO_UNIT_WRITTEN, the others
 * RO_UNIT_NO_ROOM: they carry naxis1, naxis2 and bytes, with offset 0.  SKIPPED and INVALID entries are zero but for the
 * status.  The bytes between a file's end and the next multiple of 16 are zero.  Bytes of d_png past the summary's
 * units_bytes are not touched; the sources are only read; equal inputs give equal bytes.  n == 0 is RO_OK with a zero summary.
 * Three plain launches (csrc/ro_png.hip), no atomics, no workgroup waiting for another: the plan; a workgroup per stored
 * block that writes its header and raw bytes and leaves what it adds to the two checksums in handle scratch; a wave per
 * file that adds those up and writes the Adler-32, the CRC, IEND and the pad.  Asynchronous on `stream`; the scratch is
 * this call's own (it grows, waiting for the device, with dir_capacity and with png_bytes): one call in flight per handle
 * unless they share a stream.  A chunk is ... ro_stft_snapshot_levels_resident, then this call, then one download.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, d_level_summary, d_png_dir or
 * d_png_summary; d_level_dir == NULL with dir_capacity > 0; d_levels == NULL with levels_bytes > 0; d_png == NULL with
 * png_bytes > 0; d_png not aligned to 16 bytes; a negative dir_capacity, levels_bytes or png_bytes; dir_capacity > 2^24;
 * [d_png, + png_bytes) overlapping the levels. */
int ro_stft_levels_png_resident(ro_stft_t *h, const ro_fits_unit_t *d_level_dir, int64_t dir_capacity,
                                const ro_unit_summary_t *d_level_summary, const void *d_levels, int64_t levels_bytes,
                                ro_fits_unit_t *d_png_dir, void *d_png, int64_t png_bytes,
                                ro_unit_summary_t *d_png_summary, void *stream);

/* The same rules over host memory, entry by entry, with a byte-at-a-time CRC-32 and Adler-32: no handle, no device.  The
 * yardstick of the device call: equal inputs give equal bytes in every output.  Refusals as above, without the handle and
 * the alignment. */
int ro_levels_png_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                       const void *levels, int64_t levels_bytes, ro_fits_unit_t *png_dir, void *png, int64_t png_bytes,
                       ro_unit_summary_t *png_summary);

/* ---- compressed preview files: Huffman-coded deflate blocks ---------------------------
 * The files above are as large as their pixels.  These two calls write the same files -- same signature, IHDR, one IDAT
 * with the zlib header 78 01 and the Adler-32 of the raw scanlines, IEND; filter byte 0; the raw bytes cut into blocks of
 * 65535, the last one shorter -- with every block in the shorter of two forms.  LZ77 matching and filter choice stay out of
 * scope, and so do fits2png's legend and axes.  Every block starts on a byte boundary of the stream.
 *   STORED form    the five-byte header above (BFINAL, LEN, ~LEN) and the raw bytes: 5 + LEN bytes
 *   HUFFMAN form   BTYPE = 2 with literals only.  The alphabet is the 256 literals and end-of-block (symbol 256); f[0 ... 255]
 *                  are the frequencies of the block's raw bytes and f[256] = 1, so at least two symbols are used.
 *     code lengths   The used symbols, sorted by (frequency ascending, symbol ascending), are the leaves of the two-queue
 *                  Huffman construction: leaves wait in that order, internal nodes in the order they were made, each step
 *                  joins the two smallest weights, on equal weight a leaf goes before an internal node and an earlier node
 *                  before a later one.  Of the tree only num[l], the leaves at depth l, is kept.  The limit to 15 bits:
 *                  every num[l > 15] is added into num[15]; total = sum of num[l] 2^(15 - l); while total != 2^15:
 *                  decrement num[15], take the largest l < 15 with num[l] > 0, decrement it and add 2 to num[l + 1],
 *                  decrement total.  Lengths go to the symbols in the order (frequency descending, symbol ascending):
 *                  first num[1] of them get 1, then num[2] get 2, ...; unused symbols have length 0.  The codes are the
 *                  canonical ones of RFC 1951 3.2.2.
 *     header       1106 bits: BFINAL; BTYPE = 2; HLIT = 0 (257 codes); HDIST = 0 (one distance code); HCLEN = 15 (19 entries);
 *                  the 19 three-bit code-length-code lengths in RFC order (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13,
 *                  2, 14, 1, 15): 0 for 16, 17 and 18 and 4 for 0 ... 15, so the code of a length v is v in four bits; then
 *                  258 of those four-bit codes: the 257 lengths, and 0 for the one distance code.  No run-length symbols.
 *     body         one code per raw byte, then end-of-block's
 *     ending       a block that is not the file's last: 000 (the header bits of an empty stored block), zero bits up to the
 *                  byte boundary, 00 00 FF FF.  The last block: zero bits up to the byte boundary.
 * A block takes the Huffman form exactly when that form, ending included, is shorter in bytes than 5 + LEN.  So a file is
 * never larger than ro_png_bytes(naxis1, naxis2), which stays the caller's upper bound; IDAT's length is 6 + the blocks'
 * bytes and the file's 57 more.
 * The arguments, the entry rules 1 - 3, the prefix rule and the refusals are ro_stft_levels_png_resident's (the text names
 * this call), with the sizes depending on the data: `bytes` is the file's exact size, files are packed one behind the other
 * by their ACTUAL rooms (bytes rounded up to RO_PNG_ALIGN), an entry is RO_UNIT_WRITTEN when the rooms up to and including
 * its own fit in png_bytes and RO_UNIT_NO_ROOM (with its shape and exact bytes, offset 0) otherwise, needed_bytes is the sum
 * of the actual rooms of all writable entries -- a call with d_png = NULL, png_bytes = 0 is the sizing call -- and
 * units_bytes the end of the last written file.  One more clause of rule 2: every entry is measured, fitting or not, and
 * the blocks that can be measured are bounded from the arguments, 2 (levels_bytes / 65535) + 1 + dir_capacity -- what level
 * images lying side by side in levels_bytes can have.  Counting the blocks of the entries that pass the other clauses in
 * directory order, the entries from the first one on with which the count passes that bound are RO_UNIT_INVALID (level
 * images that overlap each other many times over).
 * Six plain launches (csrc/ro_png_deflate.hip), no global atomics, no floating point, no workgroup waiting for another:
 * the entry rules and the blocks' prefix; a workgroup per block that counts its bytes, sorts the frequencies, builds the
 * code and leaves the block's size, form and code table in handle scratch; a wave per file that sums its blocks; the
 * directory and the summary; a workgroup per block of a written file that assembles the block's bits in LDS, stores them
 * and leaves what the block adds to the two checksums; a wave per file for the Adler-32, the CRC, IEND and the pad.
 * Asynchronous on `stream`; the scratch is this call's own (it grows, waiting for the device, with dir_capacity and with
 * levels_bytes): one call in flight per handle unless they share a stream. */
int ro_stft_levels_png_deflate_resident(ro_stft_t *h, const ro_fits_unit_t *d_level_dir, int64_t dir_capacity,
                                        const ro_unit_summary_t *d_level_summary, const void *d_levels, int64_t levels_bytes,
                                        ro_fits_unit_t *d_png_dir, void *d_png, int64_t png_bytes,
                                        ro_unit_summary_t *d_png_summary, void *stream);

/* The same rules over host memory, entry by entry and block by block, with a bit writer and a byte-at-a-time CRC-32 and
 * Adler-32: no handle, no device.  The yardstick of the device call: equal inputs give equal bytes in every output.
 * Refusals as above, without the handle and the alignment. */
int ro_levels_png_deflate_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                               const void *levels, int64_t levels_bytes, ro_fits_unit_t *png_dir, void *png, int64_t png_bytes,
                               ro_unit_summary_t *png_summary);

/* The directory ro_periodic_plan left, in the level form the call above reads: host arithmetic.  Entry d of level_dir
 * describes dir[d]: RO_PERIODIC_WRITTEN becomes {offset / 4, bytes = naxis1 rows, naxis2 = rows, naxis1, RO_UNIT_WRITTEN}
 * -- where ro_stft_periodic_levels_resident puts that entry's image -- RO_PERIODIC_LOST and RO_PERIODIC_NO_ROOM become
 * RO_UNIT_SKIPPED, zero but for the status.  level_summary counts them (entries, written, skipped) and has a quarter of the
 * end of the last WRITTEN unit as units_bytes and needed_bytes.  The periodic chain is ... ro_stft_periodic_levels_resident,
 * the upload of entries x 32 bytes and the summary (the caller's own copy, on the same stream), then
 * ro_stft_levels_png_resident.  RO_ERR_INVALID: a negative entries; null dir or level_dir with entries > 0; null
 * level_summary; an entry with an unknown status. */
int ro_periodic_level_dir(const ro_periodic_entry_t *dir, int64_t entries, ro_fits_unit_t *level_dir,
                          ro_unit_summary_t *level_summary);

/* ---- resized previews: fits2png's --width ----------------------------------------------
 * What a station publishes of a WIDE preview is limited to about a thousand pixels of width: fits2png:510-517 is
 * result.resize((width, int(height * ratio)), Image.ANTIALIAS), Pillow's Lanczos resize of an 8-bit image.  The calls here
 * make that image from every level image of a level directory, byte for byte what Pillow makes, and leave it as a level
 * directory again, so that ro_stft_levels_png_resident, ro_stft_levels_png_deflate_resident and their host twins read the
 * result unchanged.  A chunk is ... the levels, ro_resize_plan, the upload of the plan, ro_stft_levels_resize_resident, a
 * PNG call, one download.
 * THE PLAN IS HOST ARITHMETIC, like ro_periodic_plan: the taps come from sin in double, and they only equal Pillow's when
 * they come from the same C library -- a device sin differs in the last place often enough to flip a 22-bit tap, and then
 * a pixel.  The device does integer work only, which is also what lets it agree with its host twin byte for byte.  So the
 * shapes must be known on the host: for the periodic chain, where the wide images are, they are (ro_periodic_level_dir is
 * host memory); for the event snapshots the host downloads the level directory and its summary first, 32 bytes an entry.
 * Shape: an image is resized only when width < W = naxis1.  Then ratio = (double)width / (double)W, W' = width and
 * H' = (int64)((double)H * ratio), truncated; H' can be 0.  Otherwise it keeps its shape.
 * Coefficients of one axis (in -> out pixels, in != out), all in double: scale = in / out, fs = max(scale, 1), support =
 * 3 fs, ss = 1 / fs, ksize = (int)ceil(support) * 2 + 1.  For output pixel xx: center = (xx + 0.5) scale; xmin =
 * max((int)(center - support + 0.5), 0); xmax = min((int)(center + support + 0.5), in) - xmin; w[x] = L((x + xmin - center
 * + 0.5) ss) for x < xmax, with L(t) = sinc(t) sinc(t / 3) for -3 <= t < 3 and 0 elsewhere, sinc(0) = 1 and sinc(t) =
 * sin(pi t) / (pi t); ww = the sum of the w[x] in index order; k[x] = w[x] / ww; the fixed-point tap is (int)(k 2^22 + 0.5)
 * for k >= 0 and (int)(k 2^22 - 0.5) otherwise.
 * One pass: out = clamp((2^21 + sum over x < xmax of in[xmin + x] tap[x]) >> 22, 0, 255), the sum an int32, the shift
 * arithmetic.  The horizontal pass (W -> W' on every row) is rounded to uint8 before the vertical one (H -> H') reads it;
 * a pass whose two sizes are equal is skipped. */
typedef struct ro_resize_info {    /* 64 bytes: the host scalars of one plan */
    int64_t jobs;                  /* WRITTEN entries: one job each */
    int64_t h_items, v_items;      /* work items of the two launches */
    int64_t mid_bytes;             /* the intermediate images, W' x H bytes per job that runs both passes (handle scratch) */
    int64_t plan_bytes;            /* the plan blob: what to upload */
    int64_t reserved[3];           /* 0 */
} ro_resize_info_t;

/* The shape rule above.  Pure host.  RO_ERR_INVALID: width < 1, naxis1 < 1, naxis2 < 1, a null result. */
int ro_resize_shape(int32_t naxis1, int64_t naxis2, int32_t width, int32_t *out_naxis1, int64_t *out_naxis2);

/* The plan of one level directory.  Pure host; nothing of the levels is read.
 *   level_dir, dir_capacity, level_summary   a HOST level directory and its summary: those of
 *                    ro_stft_snapshot_levels_resident after a download, or of ro_periodic_level_dir; n = min(max(
 *                    level_summary->entries, 0), dir_capacity)
 *   levels_bytes     the room the directory's offsets are checked against
 *   width            fits2png's --width
 *   out_level_dir    room for dir_capacity entries; entry d describes level_dir[d], for d < n, in the family's form: offset
 *                    is bytes into the out levels, a multiple of RO_LEVEL_BLOCK, bytes = naxis1 naxis2 of the RESIZED image
 *   out_levels_bytes the room of the out levels
 *   out_level_summary   one entry, as the levels' calls write it: units_bytes the end of the last written image's last
 *                    block, needed_bytes the room that holds every writable one
 *   plan, plan_bytes the blob (csrc/ro_resize.h), aligned to 8 bytes: one job per WRITTEN entry -- where its pixels are and
 *                    go, its four sizes, its two tap tables -- and the tap tables with their xmin / xmax, one per distinct
 *                    (in, out) pair, shared between axes and entries.  plan = NULL with plan_bytes = 0 is the SIZING form:
 *                    everything but the blob is written, and info->plan_bytes is what the blob takes
 *   info             one entry
 * For entry d < n, in this order:
 *   1  status != RO_UNIT_WRITTEN       RO_UNIT_SKIPPED
 *   2  rule 2 of ro_stft_levels_png_resident (a shape that cannot be a PNG included: an image has fewer than 2^31 pixels)
 *                                      RO_UNIT_INVALID
 *   3  H' == 0                         RO_UNIT_SKIPPED: fits2png has no image to save
 *   4  otherwise                       WRITABLE: naxis1 = W', naxis2 = H', bytes = W' H', blocks = ceil(bytes / 720)
 * with the family's prefix rule over all writable entries: RO_UNIT_WRITTEN when offset + 720 blocks <= out_levels_bytes,
 * otherwise RO_UNIT_NO_ROOM, carrying its shape with offset 0.  An image with width >= W is a job too, a plain copy, so
 * that the out directory is complete.
 * RO_ERR_INVALID, the text naming the argument: a negative dir_capacity, levels_bytes, out_levels_bytes or plan_bytes;
 * width < 1; dir_capacity > 2^24; a null level_summary, out_level_dir, out_level_summary or info; level_dir == NULL with
 * dir_capacity > 0; plan == NULL with plan_bytes > 0; plan not aligned to 8 bytes; plan_bytes > 0 (or a plan) that is less
 * than the blob takes -- the outputs but the blob are written then, info->plan_bytes included. */
int ro_resize_plan(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                   int64_t levels_bytes, int32_t width, ro_fits_unit_t *out_level_dir, int64_t out_levels_bytes,
                   ro_unit_summary_t *out_level_summary, void *plan, int64_t plan_bytes, ro_resize_info_t *info);

/* The resized images of one plan.
 *   info             what ro_resize_plan wrote (HOST)
 *   d_plan           the caller's upload of info->plan_bytes bytes of the blob, on the same stream, aligned to 16 bytes
 *   d_levels, levels_bytes   the level images the planned directory describes, aligned to 16 bytes
 *   d_out_levels, out_levels_bytes   the resized images, aligned to 16 bytes: every job's image at its entry's offset,
 *                    zero-padded to its last 720-byte block.  Bytes past the out summary's units_bytes are not touched
 * Two plain launches (csrc/ro_resize.hip: the horizontal pass; the vertical pass, with the copies of the images that keep
 * their shape and the zero padding), no atomics, no floating point, no workgroup waiting for another: equal inputs give
 * equal bytes.  The intermediate images live in handle scratch of this call's own (it grows, waiting for the device, with
 * info->mid_bytes): one call in flight per handle unless they share a stream.  The sources are only read.  The blob is
 * the caller's memory, so the kernels check every job against the four rooms before anything of it is touched and clamp
 * every tap's bounds into its image: a job that does not fit is left out.  Asynchronous on `stream`.  info->jobs == 0
 * launches nothing.
 * RO_ERR_INVALID, before anything is launched, the text naming the argument: a null handle, info or d_plan; an info
 * with a negative field; d_levels == NULL with levels_bytes > 0; d_out_levels == NULL with out_levels_bytes > 0; d_plan,
 * d_levels or d_out_levels not aligned to 16 bytes; a negative levels_bytes or out_levels_bytes; [d_out_levels, +
 * out_levels_bytes) overlapping the levels or the plan. */
int ro_stft_levels_resize_resident(ro_stft_t *h, const ro_resize_info_t *info, const void *d_plan, const void *d_levels,
                                   int64_t levels_bytes, void *d_out_levels, int64_t out_levels_bytes, void *stream);

/* The same over host memory from the same plan, with int32 sums: no handle, no device.  The yardstick of the device
 * call: equal inputs give equal bytes.  Refusals as above, without the handle, with 8 bytes for the plan's alignment and
 * none for the images'; and a plan that is not the blob of info->plan_bytes bytes. */
int ro_levels_resize_host(const ro_resize_info_t *info, const void *plan, const void *levels, int64_t levels_bytes,
                          void *out_levels, int64_t out_levels_bytes);

/* Times `iters` back-to-back launches of the resident path with HIP events on
 * the launch stream; ms_out[i] = duration of launch i (STFT kernel + scan kernel
 * when records are requested).  kernel_ms_out (optional, 2 floats) receives the
 * average STFT-kernel-only and scan-kernel-only durations. Synchronous. */
int ro_stft_time_resident(ro_stft_t *h, const void *d_iq, int format, int64_t samples,
                          int64_t first_row, int64_t rows,
                          float *d_rows, int64_t row_stride,
                          float *d_tile, ro_scan_record_t *d_records, void *stream,
                          int iters, float *ms_out, float *kernel_ms_out);

/* ---- streaming path (the Backend::process boundary) -------------------------
 * ro_stft_push   = FFTBackend::process (src/FFTBackend.cpp:192-279): takes one
 *                  Frontend::process() call worth of samples (any count), stages
 *                  them, and runs the kernels whenever max_batch_rows rows are
 *                  complete.  *rows_ready = rows waiting in the output queue.
 * ro_stft_flush  = run the kernels on every complete row staged so far
 *                  (WaterfallBackend::endStream, src/WaterfallBackend.cpp:600-607;
 *                  samples short of a hop are dropped, like the reference).
 * ro_stft_fetch  = hand rows to the Recorder side in stream order
 *                  (replaces the synchronous Recorder::update() per row,
 *                  src/WaterfallBackend.cpp:534-536): up to max_rows rows, columns
 *                  [first_col, first_col+cols) of each, plus scan records.  With a tile
 *                  configured (tile_cols > 0) only the tile's columns travel to the host
 *                  (what the FITS writer keeps, src/WaterfallBackend.cpp:176,204) and the
 *                  requested columns must lie inside it.
 *                  *first_row_index = stream index of the first row returned. */
int ro_stft_push(ro_stft_t *h, const void *iq, int format, int64_t samples, int64_t *rows_ready);
int ro_stft_flush(ro_stft_t *h, int64_t *rows_ready);
int ro_stft_fetch(ro_stft_t *h, int64_t max_rows, int first_col, int cols,
                  float *rows_out, ro_scan_record_t *records_out,
                  int64_t *first_row_index, int64_t *rows_got);
/* ro_stft_fetch plus extra_out: host, max_rows x count records in the same row-major layout, or NULL.  (ro_stft_fetch and
 * ro_stft_fetch_ln hand out the primary record only; a batch's extra records go with its rows.) */
int ro_stft_fetch_sets(ro_stft_t *h, int64_t max_rows, int first_col, int cols, float *rows_out,
                       ro_scan_record_t *records_out, ro_scan_record_t *extra_out,
                       int64_t *first_row_index, int64_t *rows_got);
/* Tile windows on the streaming path: with windows set, each batch's rows are cut (ro_stft_cut_windows_resident's
 * kernel) behind the transform and only the image and the records travel to the host -- the recorders' own [leftBin,
 * rightBin) cuts (src/WaterfallBackend.cpp:174-205, :368-374) instead of full rows or one tile over their hull.
 * first_col / cols of ro_stft_fetch and ro_stft_fetch_sets are then IMAGE columns in [0, total), RO_ERR_INVALID outside;
 * the records stay those of the full row, in row coordinates.  count = 0 removes the windows and restores full rows.
 * The list is checked like ro_tile_windows_supported (RO_ERR_INVALID, the message names the offending window).  Only on
 * an idle stream (nothing staged, nothing waiting to be fetched), else RO_ERR_STATE; the slots' image blocks and the
 * pinned batches start over.  Refused: a handle created with a tile (tile_cols > 0) or tile_ln, RO_ERR_UNSUPPORTED; a
 * handle with a row sink, RO_ERR_STATE -- and ro_stft_set_row_sink gives RO_ERR_STATE while windows are set. */
int ro_stft_set_tile_windows(ro_stft_t *h, const ro_band_window_t *windows, int count);
int ro_stft_tile_windows(const ro_stft_t *h, ro_band_window_t *out /* may be NULL */);   /* returns count */
/* Rows at the head of the output queue whose batches have finished on the device, download included: ro_stft_fetch
 * hands these over without waiting (it WAITS for anything beyond them).  A host that fetches only what is complete
 * keeps the next batch in flight under the previous one's download and under its own per-row work -- the recorders
 * then see a batch's rows one Backend::process call later than a blocking fetch would show them, never later than the
 * next call or ro_stft_flush + fetch (src/WaterfallBackend.cpp:534-536 runs Recorder::update() inside processFFT;
 * here it runs a batch behind by construction). */
int ro_stft_rows_complete(ro_stft_t *h, int64_t *rows);
/* Row sink: the streaming path's rows go STRAIGHT into the caller's row ring instead of the handle's pinned batches --
 * WaterfallBackend::processFFT writes each finished row into buffer_->push() (src/WaterfallBackend.cpp:488-505); with a
 * sink the device-to-host copy of a batch is that write, and the ring's only copy.  Row r of the stream (counted from
 * ro_stft_create / ro_stft_reset) lands at  base + ((first_slot + r) mod capacity_rows) * row_stride  floats: the
 * handle's full rows, or its tile's columns when one is configured.  The ring has to be page-locked memory from
 * ro_pinned_alloc (the copies are asynchronous; hipPointerGetAttributes is asked about its first and last byte and
 * anything that is not a host allocation of this process's HIP runtime -- heap memory, a numpy array -- is refused with
 * RO_ERR_INVALID) and has to stay allocated until the sink is removed (base = NULL) or
 * the handle destroyed.  (ro_stft_flush launches batch by batch: one that would lap unfetched rows returns RO_ERR_STATE
 * with its samples still staged -- fetch, then flush again.)  With a sink ro_stft_push is ALL OR NOTHING: a call whose samples would complete more rows than
 * the ring has free slots (capacity_rows - rows waiting to be fetched) returns RO_ERR_STATE having consumed nothing;
 * fetch, then push the same buffer again.  A row is in place once ro_stft_fetch has reported it
 * (rows_out = NULL from then on: RO_ERR_STATE otherwise; the scan records still come through records_out), and the
 * handle writes the slots of every launched batch AHEAD of what has been fetched (as many batches as the caller lets
 * stay in flight, never lapping rows that wait to be fetched): capacity_rows >= 2 x max_batch_rows, and
 * whoever reads old rows of the ring (snapshot writers) has to stay that far behind the head, as it has to for push().
 * Only on an idle stream (RO_ERR_STATE otherwise); not for tile_ln handles (RO_ERR_UNSUPPORTED). */
int ro_stft_set_row_sink(ro_stft_t *h, float *base, int64_t row_stride, int64_t capacity_rows, int64_t first_slot);
/* page-locked host memory for such a ring (hipHostMalloc on `device`'s context); NULL when there is none to be had */
void *ro_pinned_alloc(int device, size_t bytes);
void  ro_pinned_free(void *p);
/* 1 when the first and the last byte of [p, p + bytes) are host memory page-locked by this process's HIP runtime and
 * lie the same distance apart in its view (what ro_stft_set_row_sink accepts:
 * the target of the DMA that stands in for processFFT's write into buffer_->push(), src/WaterfallBackend.cpp:488-505),
 * 0 for anything else -- heap or stack memory, device memory, or no HIP device in the process. */
int   ro_pinned_check(const void *p, size_t bytes);
/* ro_stft_fetch for a handle with tile_ln = 1: the whole tile of each row, its log, the row's min / max of the log
 * (2 floats) and the scan record -- any of the four may be NULL. */
int ro_stft_fetch_ln(ro_stft_t *h, int64_t max_rows, float *tile_out, float *ln_out, float *minmax_out,
                     ro_scan_record_t *records_out, int64_t *first_row_index, int64_t *rows_got);
/* FFTBackend::startStream's reset of inMark_/info_ (src/FFTBackend.cpp:148-153) */
int ro_stft_reset(ro_stft_t *h);
/* Per-call timing, the counterpart of FFTBackend's three RunningAverage2 counters and logProcessingTimes /
 * clearProcessingTime (src/FFTBackend.h:86-92, :208-235: average and maximum per process() call, per FFT, per
 * analysis).  push = wall time of one ro_stft_push (the host side of Backend::process); batch = GPU time of the kernels
 * of one batch (HIP events; window + FFT + magnitude, and the band scan where the plan fuses it), known once the batch
 * has been fetched; row = the same per row; fetch = wall time of one ro_stft_fetch (includes waiting for the GPU).
 * `batches` / `batch_rows` count every batch; of the latency-bound batches that run as one captured graph (full batches of
 * at most 4 MiB into a row sink) one in eight carries the timing events -- an event record costs the host as much as a
 * kernel launch -- and batch_gpu_ms_avg / _max and row_gpu_us_avg are over the timed ones. */
typedef struct ro_stft_timing {
    int64_t push_calls;  double push_ms_avg, push_ms_max;
    int64_t batches;     double batch_gpu_ms_avg, batch_gpu_ms_max;
    int64_t batch_rows;  double row_gpu_us_avg;
    int64_t fetch_calls; double fetch_ms_avg, fetch_ms_max;
} ro_stft_timing_t;
int ro_stft_timing(ro_stft_t *h, ro_stft_timing_t *out, int reset /* != 0: clear the counters afterwards */);
/* totals in the spirit of FFTBackend::logProcessingTimes (src/FFTBackend.h:208-229); kernel_ms_total counts an untimed
 * graphed batch (see ro_stft_timing) with the time of the last timed one -- the same graph */
int ro_stft_stats(const ro_stft_t *h, int64_t *samples_in, int64_t *rows_out,
                  int64_t *launches, double *kernel_ms_total);

#ifdef __cplusplus
}
#endif
#endif /* RO_STFT_H */
