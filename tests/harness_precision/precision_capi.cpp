// precision_capi.cpp -- plain-C shim over the product's host-side C++ objects (radio-observer_amd/host/, linked as
// libro_host.so) with the knobs of WaterfallConfig::precision: the "waterfall" factory's key parser, the
// Frontend -> HipWaterfallBackend -> {SnapshotRecorder, BolidRecorder} pipeline, the WAV -> FITS run and the
// Backend::process rate rig, each with a precision argument.  For tests/precisionlib.py (tests/test_precision_cpu.py,
// tests/test_gpu_precision*.py) and tools/stream_rate_precision.py.  Test infrastructure: not part of the product.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "BolidRecorder.h"
#include "Frontends.h"
#include "HipWaterfallBackend.h"
#include "SnapshotRecorder.h"

using namespace ro;

namespace {

// "key=value" lines -> the map the factory glue hands to parseWaterfallKeys
std::map<std::string, std::string> parseLines(const char *text)
{
    std::map<std::string, std::string> m;
    std::istringstream in(text ? text : "");
    std::string line;
    while (std::getline(in, line)) {
        const size_t eq = line.find('=');
        if (eq != std::string::npos) m[line.substr(0, eq)] = line.substr(eq + 1);
    }
    return m;
}

struct Rig {
    HipWaterfallBackend backend;
    SnapshotRecorder snap;
    BolidRecorder bolid;
    FrontendDriver frontend;
    Rig(const WaterfallConfig &w, const BolidConfig &b, const SnapshotConfig &sc, bool with_snapshot)
        : backend(w), snap(&backend, sc), bolid(&backend, b), frontend(&backend)
    {
        if (with_snapshot) backend.addRecorder(&snap);       // same order as radio-observer.json:52-88
        backend.addRecorder(&bolid);
        backend.keepRowLog(true);
    }
};
#define PIPE(p) static_cast<Rig *>(p)

int joinNames(const std::vector<std::string> &v, char *buf, int len)
{
    std::string all;
    for (const auto &f : v) all += f + "\n";
    std::snprintf(buf, (size_t)len, "%s", all.c_str());
    return (int)v.size();
}

}  // namespace

extern "C" {

// ---- parseWaterfallKeys over "key=value\n" text.  out_i: bins, overlap, buffer_chunk_size, iq_phase_shift, precision;
// out_d: iq_gain; origin / metadata_path as text.  Returns 1 (parsed) or 0 (refused, the reason in err).
int ro_prec_parse_keys(const char *text, int *out_i5, double *out_gain, char *origin, int origin_len, char *meta,
                       int meta_len, char *err, int err_len)
{
    WaterfallConfig c;
    std::string why;
    const bool ok = parseWaterfallKeys(parseLines(text), &c, &why);
    out_i5[0] = c.bins; out_i5[1] = c.overlap; out_i5[2] = c.buffer_chunk_size; out_i5[3] = c.iq_phase_shift;
    out_i5[4] = c.precision;
    *out_gain = c.iq_gain;
    std::snprintf(origin, (size_t)origin_len, "%s", c.origin.c_str());
    std::snprintf(meta, (size_t)meta_len, "%s", c.metadata_path.c_str());
    std::snprintf(err, (size_t)err_len, "%s", why.c_str());
    return ok ? 1 : 0;
}
int ro_prec_default_precision() { return WaterfallConfig().precision; }

// ---- Frontend -> HipWaterfallBackend -> [SnapshotRecorder] -> BolidRecorder.  out_dir == nullptr: the detector only,
// no files, detect / noise bands and times as given; else a SnapshotRecorder of [lo_snap, hi_snap) Hz and a detector
// on radio-observer.json's bands, both writing FITS files under out_dir.
void *ro_prec_pipeline_create(int precision, int bins, int overlap, int sample_rate, int64_t start_sec, int64_t start_usec,
                              int max_batch_rows, int snapshot_length, float lo_det, float hi_det, float lo_noise,
                              float hi_noise, double advance_time, double jitter_time, float avg_range, float lo_snap,
                              float hi_snap, const char *out_dir, const char *origin)
{
    WaterfallConfig w;
    w.bins = bins;
    w.overlap = overlap;
    w.max_batch_rows = max_batch_rows;
    w.precision = precision;
    w.metadata_path = out_dir ? out_dir : "";
    if (origin) w.origin = origin;
    BolidConfig b;
    b.snapshot_length = snapshot_length;
    b.low_detect_freq = lo_det; b.hi_detect_freq = hi_det; b.low_noise_freq = lo_noise; b.hi_noise_freq = hi_noise;
    b.advance_time = advance_time; b.jitter_time = jitter_time; b.avg_freq_range = avg_range;
    SnapshotConfig sc;
    if (out_dir) {
        b.output_dir = out_dir;
        sc.output_dir = out_dir;
        sc.snapshot_length = snapshot_length;
        sc.low_freq = lo_snap;
        sc.hi_freq = hi_snap;
    } else {
        b.write_files = false;
    }
    Rig *p = new Rig(w, b, sc, out_dir != nullptr);
    StreamInfo si;
    si.sampleRate = sample_rate;
    si.timeOffset = WFTime(start_sec, start_usec);
    p->frontend.startStream(si);
    return p;
}
void ro_prec_pipeline_destroy(void *p) { delete PIPE(p); }
void ro_prec_pipeline_set_clock(void *p, int64_t sec, int64_t usec) { PIPE(p)->backend.setClock(WFTime(sec, usec)); }
// one Frontend::process() call: n complex doubles (struct Complex)
void ro_prec_pipeline_process(void *p, const double *iq, int n)
{
    std::vector<Complex> v((size_t)n);
    std::memcpy(v.data(), iq, sizeof(Complex) * (size_t)n);
    PIPE(p)->frontend.process(v);
}
void ro_prec_pipeline_end(void *p) { PIPE(p)->frontend.endStream(); }
int64_t ro_prec_pipeline_rows(void *p) { return PIPE(p)->backend.rowsDelivered(); }
const char *ro_prec_pipeline_error(void *p) { return PIPE(p)->backend.lastError().c_str(); }
int ro_prec_pipeline_precision(void *p) { return PIPE(p)->backend.config().precision; }
int ro_prec_pipeline_ring_capacity(void *p) { return PIPE(p)->backend.buffer().getCapacity(); }
int ro_prec_pipeline_ring_mark(void *p) { return PIPE(p)->backend.buffer().mark(); }
int ro_prec_pipeline_raw_capacity(void *p) { return PIPE(p)->backend.rawCapacity(); }
int ro_prec_pipeline_raw_mark(void *p) { return PIPE(p)->backend.rawBuffer().mark(); }
int ro_prec_pipeline_batch_rows(void *p) { return PIPE(p)->backend.batchRows(); }
int ro_prec_pipeline_state(void *p) { return (int)PIPE(p)->bolid.state(); }
void ro_prec_pipeline_ring_row(void *p, int mark, float *out)
{
    std::memcpy(out, PIPE(p)->backend.buffer().at(mark), sizeof(float) * (size_t)PIPE(p)->backend.getBins());
}
// the whole raw I/Q ring in slot order (rawCapacity() float pairs)
int ro_prec_pipeline_raw_ring(void *p, float *out2, int max)
{
    RingBuffer2D<float> &r = PIPE(p)->backend.rawBuffer();
    const int n = std::min(r.getCapacity(), max);
    for (int i = 0; i < n; ++i) {
        const float *s = r.at(i);
        out2[2 * i] = s[0];
        out2[2 * i + 1] = s[1];
    }
    return r.getCapacity();
}
int ro_prec_pipeline_row_info(void *p, int64_t i, uint64_t *offset, int64_t *sec, int64_t *usec, int *raw_mark)
{
    const auto &log = PIPE(p)->backend.rowLog();
    if (i < 0 || i >= (int64_t)log.size()) return -1;
    *offset = log[(size_t)i].offset;
    *sec = log[(size_t)i].time.sec;
    *usec = log[(size_t)i].time.usec;
    *raw_mark = log[(size_t)i].rawMark;
    return 0;
}
void ro_prec_pipeline_raw_handle(void *p, int mark, int *raw_mark, int64_t *sec, int64_t *usec)
{
    const auto &h = PIPE(p)->backend.rawHandles();
    const RawDataHandle &x = h[(size_t)mark % h.size()];
    *raw_mark = x.mark;
    *sec = x.time.sec;
    *usec = x.time.usec;
}
void ro_prec_pipeline_bands(void *p, int *out7)
{
    const BolidRecorder &b = PIPE(p)->bolid;
    out7[0] = b.lowDetectBin(); out7[1] = b.detectWidth(); out7[2] = b.lowNoiseBin(); out7[3] = b.noiseWidth();
    out7[4] = b.advance(); out7[5] = b.jitter(); out7[6] = b.averageBinRange();
}
int ro_prec_pipeline_events(void *p, BolidEvent *out, int max)
{
    const auto &ev = PIPE(p)->bolid.events();
    const int n = (int)std::min<size_t>(ev.size(), (size_t)max);
    for (int i = 0; i < n; ++i) out[i] = ev[(size_t)i];
    return (int)ev.size();
}
// files written: kind 0 the SnapshotRecorder's, 1 the detector's band snapshots ("blid"), 2 its raw I/Q captures ("raws")
int ro_prec_pipeline_files(void *p, int kind, char *buf, int len)
{
    if (kind == 0) return joinNames(PIPE(p)->snap.filesWritten(), buf, len);
    const BolidRecorder &b = PIPE(p)->bolid;
    return joinNames(kind == 2 ? b.rawFilesWritten() : b.filesWritten(), buf, len);
}
// ro_stft_timing of the stream's handle: out6 = push calls, push ms avg, batches, batch GPU ms avg, fetch calls, fetch ms avg
int ro_prec_pipeline_timing(void *p, double *out6)
{
    ro_stft_timing_t t;
    std::memset(&t, 0, sizeof t);
    if (!PIPE(p)->backend.timing(&t, false)) return -1;
    out6[0] = (double)t.push_calls; out6[1] = t.push_ms_avg; out6[2] = (double)t.batches;
    out6[3] = t.batch_gpu_ms_avg; out6[4] = (double)t.fetch_calls; out6[5] = t.fetch_ms_avg;
    return 0;
}

// ---- C1 end to end: WAV bytes -> WAVStream -> HipWaterfallBackend (GPU) -> SnapshotRecorder -> FITS files.
// clock_sec >= 0 pins WFTime::now() (the DATE card).
int64_t ro_prec_wav_to_fits(int precision, const char *bytes, int64_t n, int bins, int overlap, int max_batch_rows,
                            int snapshot_length, float lo, float hi, const char *out_dir, const char *origin,
                            int64_t clock_sec, char *files, int files_len, char *err, int err_len)
{
    WaterfallConfig w;
    w.bins = bins;
    w.overlap = overlap;
    w.max_batch_rows = max_batch_rows;
    w.precision = precision;
    w.origin = origin;
    w.metadata_path = out_dir;
    SnapshotConfig sc;
    sc.output_dir = out_dir;
    sc.snapshot_length = snapshot_length;
    sc.low_freq = lo;
    sc.hi_freq = hi;
    HipWaterfallBackend backend(w);
    if (clock_sec >= 0) backend.setClock(WFTime(clock_sec, 0));
    SnapshotRecorder snap(&backend, sc);
    backend.addRecorder(&snap);
    std::istringstream in(std::string(bytes, (size_t)n));
    WAVStream wav(in);
    ro::Pipeline pipe;                                   // Frontend -> Pipeline -> Backend, as in the reference's main()
    pipe.setFrontend(&wav);
    pipe.setBackend(&backend);
    pipe.run();
    const bool ok = wav.ok();
    joinNames(snap.filesWritten(), files, files_len);
    std::snprintf(err, (size_t)err_len, "%s%s", ok ? "" : wav.lastError().c_str(), backend.lastError().c_str());
    return backend.rowsDelivered();
}

// ---- rows/s through Backend::process: Frontend::process -> HipWaterfallBackend::process -> BolidRecorder::update per
// row, `block` samples of vector<Complex> per call (src/RawStream.cpp:44-66), for `seconds` after `warm_calls` untimed
// calls.  The samples are sigma = 1 doubles with low-order bits float32 cannot hold.
// stats: [0] seconds  [1] samples  [2] rows delivered  [3] process() calls  [4] rows per kernel launch
//        [5] mean ms per process() call  [6] max ms per process() call  [7] events fired
//        [8] push ms avg  [9] fetch ms avg  [10] batch GPU ms avg  [11] row GPU us avg  [12] push calls  [13] fetch calls
//        [14] batches  [15] rows by DMA (1/0)
int ro_prec_stream_bench(int precision, int bins, int overlap, int sample_rate, int block, double seconds,
                         int max_batch_rows, int warm_calls, double *stats)
{
    if (bins <= 0 || block <= 0 || seconds <= 0 || !stats) return -1;
    WaterfallConfig w;
    w.bins = bins;
    w.overlap = overlap;
    w.max_batch_rows = max_batch_rows;
    w.precision = precision;
    w.metadata_path = "";
    BolidConfig b;                                   // radio-observer.json:62-87
    b.snapshot_length = 60;
    b.low_detect_freq = 10300; b.hi_detect_freq = 10900; b.low_noise_freq = 9000; b.hi_noise_freq = 9600;
    b.advance_time = 2; b.jitter_time = 5; b.avg_freq_range = 40;
    b.write_files = false;
    HipWaterfallBackend backend(w);
    BolidRecorder bolid(&backend, b);
    backend.addRecorder(&bolid);
    FrontendDriver frontend(&backend);
    // two blocks alternate (a frontend refills ONE vector per call: what Backend::process reads is cache-hot)
    std::vector<std::vector<Complex>> blocks(2, std::vector<Complex>((size_t)block));
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto uni = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) * (1.0 / 9007199254740992.0); };
    for (auto &blk : blocks)
        for (auto &c : blk) {
            const double u1 = uni() + 1e-300, u2 = uni();
            const double r = std::sqrt(-2.0 * std::log(u1));
            c.real = r * std::cos(6.283185307179586 * u2) + 1e-9;
            c.imag = r * std::sin(6.283185307179586 * u2) - 1e-9;
        }
    StreamInfo si;
    si.sampleRate = sample_rate;
    frontend.startStream(si);
    if (!backend.lastError().empty()) return -2;
    int64_t calls = 0;
    for (int i = 0; i < warm_calls; ++i) frontend.process(blocks[(size_t)(calls++ % 2)]);
    const int64_t rows0 = backend.rowsDelivered();
    ro_stft_timing_t tm;
    backend.timing(&tm, true);                                       // the counters of the timed region only
    auto now = []() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; };
    const double t0 = now();
    double worst = 0.0;
    int64_t timed = 0;
    for (;;) {
        const double a = now();
        frontend.process(blocks[(size_t)(calls++ % 2)]);
        const double d = now() - a;
        worst = d > worst ? d : worst;
        ++timed;
        if (a + d - t0 >= seconds) break;
    }
    std::memset(&tm, 0, sizeof tm);
    backend.timing(&tm, false);
    frontend.endStream();
    const double dt = now() - t0;
    stats[8] = tm.push_ms_avg;  stats[9] = tm.fetch_ms_avg;  stats[10] = tm.batch_gpu_ms_avg;  stats[11] = tm.row_gpu_us_avg;
    stats[12] = (double)tm.push_calls;  stats[13] = (double)tm.fetch_calls;  stats[14] = (double)tm.batches;
    stats[15] = backend.rowsByDma() ? 1.0 : 0.0;
    stats[0] = dt;
    stats[1] = (double)timed * (double)block;
    stats[2] = (double)(backend.rowsDelivered() - rows0);
    stats[3] = (double)timed;
    stats[4] = (double)backend.batchRows();
    stats[5] = 1e3 * dt / (double)timed;
    stats[6] = 1e3 * worst;
    stats[7] = (double)bolid.events().size();
    return backend.lastError().empty() ? 0 : -3;
}

}  // extern "C"
