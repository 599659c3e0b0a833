// ro_abi_helpers.cpp -- the part of the C ABI (include/ro_stft.h) that needs no handle: the error text, FFTBackend's public
// arithmetic, the window tables, the shard arithmetic of the time-chunk split and its exchange schedule, pinned memory.
#include "ro_host.h"

namespace ro {
namespace host {

namespace {
thread_local std::string g_error;
}

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

const char *last_error_text() { return g_error.c_str(); }

// window tables: same arithmetic as FFTBackend::startStream (src/FFTBackend.cpp:156-186):
// float coefficients, double pi = 4*atan(1), (float)i and (float)(bins-1) widened to double,
// evaluation in double, one narrowing on store.
void build_window(int kind, int bins, float *w)
{
    const double pi = 4.0 * std::atan(1.0);
    const double denom = (double)(float)(bins - 1);
    if (kind == RO_WINDOW_HANN) {
        for (int i = 0; i < bins; ++i)
            w[i] = (float)(0.5 * (1.0 - std::cos(2.0 * pi * (double)(float)i / denom)));
        return;
    }
    const float a0 = 0.355768f, a1 = 0.487396f, a2 = 0.144232f, a3 = 0.012604f;
    for (int i = 0; i < bins; ++i) {
        const double x = (double)(float)i;
        w[i] = (float)((double)a0 - (double)a1 * std::cos(2.0 * pi * x / denom) +
                       (double)a2 * std::cos(4.0 * pi * x / denom) -
                       (double)a3 * std::cos(6.0 * pi * x / denom));
    }
}

// tile windows: nullptr if the list is valid, otherwise why not (*which: the offending window, -1: the list itself);
// *total: the columns in all
const char *tile_windows_fault(int bins, const ro_band_window_t *w, int count, int64_t *total, int *which)
{
    *total = 0;
    *which = -1;
    if (!w) return "null windows";
    if (count < 1 || count > RO_MAX_TILE_WINDOWS) return "a call takes 1 ... 8 windows";
    for (int i = 0; i < count; ++i) {
        *which = i;
        if (w[i].cols < 1) return "needs at least one column";
        if (w[i].first_col < 0 || (int64_t)w[i].first_col + w[i].cols > bins) return "lies outside the row";
        if (i > 0 && w[i].first_col < (int64_t)w[i - 1].first_col + w[i - 1].cols)
            return "starts before the one in front of it ends (ascending, not overlapping)";
        *total += w[i].cols;
    }
    *which = -1;
    return nullptr;
}

// the same as a refusal: RO_ERR_INVALID, the message names the offending window
int tile_windows_check(const char *who, int bins, const ro_band_window_t *w, int count, int64_t *total)
{
    int which = -1;
    const char *why = tile_windows_fault(bins, w, count, total, &which);
    if (!why) return RO_OK;
    if (which < 0) return fail(RO_ERR_INVALID, "%s: %s (%d windows of a %d-bin row)", who, why, count, bins);
    return fail(RO_ERR_INVALID, "%s: window %d, columns [%d,+%d) of a %d-bin row, %s", who, which, w[which].first_col,
                w[which].cols, bins, why);
}

ro::CutArgs make_cut_args(const ro_band_window_t *w, int count, float *d_image, int64_t image_stride)
{
    ro::CutArgs c{};
    c.image = d_image;
    c.image_stride = image_stride;
    c.count = count;
    for (int i = 0; i < count; ++i) {
        c.first[i] = w[i].first_col;
        c.off[i] = c.total;
        c.total += w[i].cols;
    }
    return c;
}

}  // namespace host
}  // namespace ro

using namespace ro::host;

// ---------------------------------------------------------------------------
// library
// ---------------------------------------------------------------------------
extern "C" int ro_abi_version(void) { return RO_ABI_VERSION; }

extern "C" const char *ro_last_error(void) { return last_error_text(); }

extern "C" int ro_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(RO_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

// ---------------------------------------------------------------------------
// host helpers (FFTBackend's scalar arithmetic; float/double mixing as in the reference)
// ---------------------------------------------------------------------------
extern "C" int ro_clamp_overlap(int bins, int overlap)
{
    if (overlap < 0) return 0;                       // src/FFTBackend.cpp:108
    if (overlap >= bins) return bins - 1;            // :109
    return overlap;
}

extern "C" float ro_fft_sample_rate(int sample_rate, int bins, int overlap)
{
    return (float)sample_rate / (float)(bins - ro_clamp_overlap(bins, overlap));   // :150-151
}

extern "C" int ro_frequency_to_bin(int bins, int sample_rate, float frequency)
{
    // src/FFTBackend.h:169-175: float quotient, double sum and product, truncation, clamp
    const float sr = (float)sample_rate, n = (float)bins;
    const int bin = (int)((double)n * ((double)(frequency / sr) + 0.5));
    if (bin < 0) return 0;
    if (bin >= bins) return bins - 1;
    return bin;
}

extern "C" float ro_bin_to_frequency(int bins, int sample_rate, int bin)
{
    // src/FFTBackend.h:141-145: float quotient, the rest in double, narrowed on return
    const float b = (float)bin, sr = (float)sample_rate, n = (float)bins;
    return (float)((double)sr * (-0.5 + (double)(b / n)));
}

extern "C" int ro_time_to_fft_samples(double seconds, float fft_sample_rate)
{
    return (int)(seconds * (double)fft_sample_rate);             // src/FFTBackend.h:197-200
}

extern "C" int64_t ro_row_count(int64_t samples, int bins, int overlap)
{
    const int64_t hop = bins - ro_clamp_overlap(bins, overlap);
    if (samples < bins) return 0;
    return (samples - bins) / hop + 1;
}

extern "C" int ro_window_table(int kind, int bins, float *out)
{
    if (!out || bins < 2) return fail(RO_ERR_INVALID, "ro_window_table: bad arguments");
    if (kind != RO_WINDOW_NUTTALL && kind != RO_WINDOW_HANN)
        return fail(RO_ERR_INVALID, "ro_window_table: kind %d has no formula", kind);
    build_window(kind, bins, out);
    return RO_OK;
}

// ---------------------------------------------------------------------------
// time-chunk sharding (host arithmetic; the Python side, timeshard.py, calls these)
// ---------------------------------------------------------------------------
extern "C" int ro_shard_rows(int64_t total_rows, int world, int rank, int64_t *first_row, int64_t *rows)
{
    if (total_rows < 0 || world < 1 || rank < 0 || rank >= world || !first_row || !rows)
        return fail(RO_ERR_INVALID, "ro_shard_rows: bad arguments");
    // 128-bit products: rank * total_rows overflows int64 only for absurd sizes, but costs nothing to rule out
    const int64_t lo = (int64_t)(((__int128)rank * total_rows) / world);
    const int64_t hi = (int64_t)(((__int128)(rank + 1) * total_rows) / world);
    *first_row = lo;
    *rows = hi - lo;
    return RO_OK;
}

extern "C" int ro_shard_samples(int64_t first_row, int64_t rows, int bins, int overlap, int64_t *first_sample,
                                int64_t *samples)
{
    if (first_row < 0 || rows < 0 || bins < 2 || !first_sample || !samples)
        return fail(RO_ERR_INVALID, "ro_shard_samples: bad arguments");
    const int64_t hop = bins - ro_clamp_overlap(bins, overlap);
    *first_sample = first_row * hop;
    *samples = rows > 0 ? (rows - 1) * hop + bins : 0;
    return RO_OK;
}

extern "C" int64_t ro_shard_max_rows(int64_t total_rows, int world)
{
    if (total_rows < 0 || world < 1) return fail(RO_ERR_INVALID, "ro_shard_max_rows: bad arguments");
    return (total_rows + world - 1) / world;       // sizes differ by at most one: the largest is the ceiling
}

extern "C" int ro_direct_schedule(int world, int rank, int64_t total_rows, int k, int *to, int *from, int64_t *recv_first_row,
                                  int64_t *recv_rows)
{
    if (world < 1 || rank < 0 || rank >= world || total_rows < 0 || k < 0 || k >= world || !to || !from || !recv_first_row ||
        !recv_rows)
        return fail(RO_ERR_INVALID, "ro_direct_schedule: bad arguments");
    *to = (rank + k) % world;
    *from = (rank - k + world) % world;
    return ro_shard_rows(total_rows, world, *from, recv_first_row, recv_rows);
}

extern "C" int ro_stitch_rows(const void *gathered, int64_t total_rows, int world, size_t row_bytes, void *out)
{
    if (total_rows < 0 || world < 1 || (total_rows > 0 && (!gathered || !out)))
        return fail(RO_ERR_INVALID, "ro_stitch_rows: bad arguments");
    const int64_t block = ro_shard_max_rows(total_rows, world);
    const char *src = static_cast<const char *>(gathered);
    char *dst = static_cast<char *>(out);
    for (int g = 0; g < world; ++g) {
        int64_t first = 0, rows = 0;
        ro_shard_rows(total_rows, world, g, &first, &rows);
        std::memcpy(dst + (size_t)first * row_bytes, src + (size_t)g * (size_t)block * row_bytes,
                    (size_t)rows * row_bytes);
    }
    return RO_OK;
}

// ---------------------------------------------------------------------------
// tile windows (host arithmetic): what several recorders keep of a row, src/WaterfallBackend.cpp:174-205, :368-374
// ---------------------------------------------------------------------------
extern "C" int ro_tile_windows_supported(int bins, const ro_band_window_t *windows, int count)
{
    int64_t total = 0;
    int which = -1;
    if (bins < 1 || !ro_bins_supported(bins)) return 0;
    return tile_windows_fault(bins, windows, count, &total, &which) ? 0 : 1;
}

extern "C" int ro_merge_windows(const ro_band_window_t *ranges, int range_count, int bins, ro_band_window_t *windows_out,
                                int *count_out, int32_t *offsets_out)
{
    if (!ranges || !windows_out || !count_out) return fail(RO_ERR_INVALID, "ro_merge_windows: null argument");
    if (range_count < 1 || range_count > 32) return fail(RO_ERR_INVALID, "ro_merge_windows: %d ranges: 1 ... 32", range_count);
    std::vector<std::pair<int64_t, int64_t>> iv;        // [lo, hi)
    for (int i = 0; i < range_count; ++i) {
        if (ranges[i].cols < 1)
            return fail(RO_ERR_INVALID, "ro_merge_windows: range %d has %d columns: at least one", i, ranges[i].cols);
        if (ranges[i].first_col < 0 || (int64_t)ranges[i].first_col + ranges[i].cols > bins)
            return fail(RO_ERR_INVALID, "ro_merge_windows: range %d, columns [%d,+%d), leaves the row [0,%d)", i,
                        ranges[i].first_col, ranges[i].cols, bins);
        iv.emplace_back(ranges[i].first_col, (int64_t)ranges[i].first_col + ranges[i].cols);
    }
    std::sort(iv.begin(), iv.end());
    std::vector<std::pair<int64_t, int64_t>> m;
    for (const auto &x : iv) {
        if (!m.empty() && x.first <= m.back().second) m.back().second = std::max(m.back().second, x.second);
        else m.push_back(x);
    }
    while ((int)m.size() > RO_MAX_TILE_WINDOWS) {       // the smallest gap goes; the lower pair on a tie (ro_bands_windows)
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
    if (offsets_out)
        for (int i = 0; i < range_count; ++i) {         // every range lies whole inside exactly one window
            int64_t off = 0;
            for (const auto &x : m) {
                if (ranges[i].first_col >= x.first && ranges[i].first_col < x.second) {
                    offsets_out[i] = (int32_t)(off + ranges[i].first_col - x.first);
                    break;
                }
                off += x.second - x.first;
            }
        }
    return RO_OK;
}

// ---------------------------------------------------------------------------
// the detector on the host: BolidRecorder::update's decision and state machine (src/BolidRecorder.cpp:135, :171-267) in
// the closed form of include/ro_stft.h, one row at a time.  ro_events.hip computes the same as a scan.
// ---------------------------------------------------------------------------
static_assert(sizeof(ro_detector_t) == 8 && sizeof(ro_event_t) == 40 && sizeof(ro_detect_state_t) == 32 &&
                  sizeof(ro_detect_summary_t) == 24, "the detector's structs are ABI");

extern "C" int ro_events_host(const ro_scan_record_t *records, int64_t record_stride, int64_t first_row, int64_t rows,
                              const ro_detector_t *det, ro_detect_state_t *state, ro_event_t *events, int64_t capacity,
                              ro_detect_summary_t *summary, uint8_t *detect)
{
    if (!det || !state) return fail(RO_ERR_INVALID, "ro_events_host: null %s", !det ? "detector" : "state");
    if (det->advance < 0 || det->jitter < 0)
        return fail(RO_ERR_INVALID, "ro_events_host: advance %d, jitter %d: neither may be negative", det->advance, det->jitter);
    if (rows < 0 || capacity < 0)
        return fail(RO_ERR_INVALID, "ro_events_host: rows %lld, capacity %lld: neither may be negative", (long long)rows,
                    (long long)capacity);
    if (capacity > 0 && !events) return fail(RO_ERR_INVALID, "ro_events_host: null events with capacity %lld", (long long)capacity);
    if (rows > 0 && (!records || record_stride < 1))
        return fail(RO_ERR_INVALID, "ro_events_host: %s", !records ? "null records" : "record_stride < 1");
    ro_detect_summary_t sum{};
    if (rows == 0) {
        if (summary) *summary = sum;
        return RO_OK;
    }
    const int64_t G = det->jitter > 2 ? det->jitter : 2;
    ro_detect_state_t st = *state;
    // a group that could no longer fire (rows were left out between two calls) is closed silently
    if (st.open && st.last_detect_row + G < first_row) st.open = 0;
    for (int64_t i = 0; i < rows; ++i) {
        const ro_scan_record_t &rec = records[i * record_stride];
        const int64_t r = first_row + i;
        const double n = (double)rec.noise, a = (double)rec.average;
        const bool d = a > n * 2.0;                                     // :135
        if (std::fabs(a / (2.0 * n) - 1.0) <= 1e-5) sum.marginal_rows += 1;
        if (detect) detect[i] = d ? 1 : 0;
        if (d) {
            sum.detect_rows += 1;
            if (!st.open) {                                             // STATE_INIT -> STATE_BOLID, :173-182
                st.open = 1;
                st.first_detect_row = r;
                st.noise = rec.noise;
                st.peak = rec.peak;
                st.magnitude = rec.average;
            }
            st.last_detect_row = r;                                     // STATE_BOLID, or back to it (:186-187, :198-199)
        } else if (st.open && r == st.last_detect_row + G) {            // duration_ >= jitter_, :201-264
            if (sum.events < capacity) {
                ro_event_t &e = events[sum.events];
                e.fire_row = r;
                e.start_row = st.first_detect_row + 1 - det->advance;
                e.length = 2 * (int64_t)det->advance + (st.last_detect_row - st.first_detect_row + 1);
                e.noise = st.noise;
                e.peak = st.peak;
                e.magnitude = st.magnitude;
                e.reserved = 0;
            }
            sum.events += 1;
            st.open = 0;
        }
    }
    if (!st.open) st = ro_detect_state_t{};                             // every state that is not open is all zero
    else st.open = 1;
    *state = st;
    if (summary) *summary = sum;
    return RO_OK;
}

extern "C" int ro_ln_levels(const float *ln, int64_t count, float mn, float mx, uint8_t *levels_out)
{
    if (count < 0 || (count > 0 && (!ln || !levels_out))) return fail(RO_ERR_INVALID, "ro_ln_levels: bad arguments");
    const float span = mx - mn;
    for (int64_t i = 0; i < count; ++i) {
        // float32 throughout, like numpy in the viewer (fits2png:444-445); -inf = a zero pixel (dropped there)
        const float level = (ln[i] - mn) / span * 255.f;
        levels_out[i] = (std::isfinite(ln[i]) && span > 0.f) ? (uint8_t)(int)level : (uint8_t)0;
    }
    return RO_OK;
}

// 1: [p, p + bytes) is host memory page-locked by this process's HIP runtime (ro_pinned_alloc, hipHostMalloc,
// hipHostRegister) -- first and last byte are both known to the runtime as host allocations and lie in ONE mapping
// (equal distance in the runtime's view); 0: it is not (heap, stack, a numpy array, device memory, no device at all).
extern "C" int ro_pinned_check(const void *p, size_t bytes)
{
    if (!p || bytes == 0) return 0;
    const char *lo = static_cast<const char *>(p), *hi = lo + bytes - 1;
    hipPointerAttribute_t a0{}, a1{};
    const hipError_t e0 = hipPointerGetAttributes(&a0, lo);
    const hipError_t e1 = e0 == hipSuccess ? hipPointerGetAttributes(&a1, hi) : e0;
    if (e0 != hipSuccess || e1 != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return a0.type == hipMemoryTypeHost && a1.type == hipMemoryTypeHost && a0.hostPointer && a1.hostPointer &&
                   static_cast<const char *>(a1.hostPointer) - static_cast<const char *>(a0.hostPointer) == hi - lo
               ? 1 : 0;
}

extern "C" void *ro_pinned_alloc(int device, size_t bytes)
{
    void *p = nullptr;
    if (bytes == 0 || hipSetDevice(device) != hipSuccess) return nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

extern "C" void ro_pinned_free(void *p)
{
    if (p) (void)hipHostFree(p);
}
