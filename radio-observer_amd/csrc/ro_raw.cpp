// ro_raw.cpp -- the raw I/Q of each event, cut from the resident samples (include/ro_stft.h; kernels: ro_raw.hip): argument
// checks, the handle's scratch, the launches; and ro_raw_host, the same rules candidate by candidate over host memory.
// Nothing in the resident call reads device memory: which events there are, which of their samples the spans still hold
// and where they go in the arena are decided on the device.
#include "ro_host.h"

using namespace ro::host;

static_assert(sizeof(ro_iq_span_t) == 32 && sizeof(ro_raw_capture_t) == 72 && sizeof(ro_raw_summary_t) == 64,
              "the raw capture's structs are ABI");

namespace {

// what ro_raw_host and ro_stft_raw_resident ask of their common arguments, as a refusal in the name of `who`; d: "d_" where
// the arrays are the device's (the argument names of the resident call), "" on the host; aligned: the device's loads and
// stores are 8 bytes wide (4 for RO_IQ_I16 samples)
int raw_check(const char *who, const char *d, bool aligned, const ro_snapshot_t *dir, int64_t dir_capacity,
              const ro_snap_summary_t *snap_summary, const ro_iq_span_t *spans, int span_count, const ro_snapshot_t *pending,
              const int64_t *pending_count, int64_t pending_capacity, const ro_raw_capture_t *raw_dir, const float *arena,
              int64_t arena_floats, const ro_raw_summary_t *raw_summary)
{
    if (dir_capacity < 0 || pending_capacity < 0 || arena_floats < 0)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld, pending_capacity %lld, arena_floats %lld: none may be negative", who,
                    (long long)dir_capacity, (long long)pending_capacity, (long long)arena_floats);
    if (!snap_summary) return fail(RO_ERR_INVALID, "%s: null %ssnap_summary", who, d);
    if (dir_capacity > 0 && !dir) return fail(RO_ERR_INVALID, "%s: null %sdir with dir_capacity %lld", who, d, (long long)dir_capacity);
    if (!spans) return fail(RO_ERR_INVALID, "%s: null spans", who);
    if (span_count < 1 || span_count > RO_MAX_IQ_SPANS)
        return fail(RO_ERR_INVALID, "%s: span_count %d: a call takes 1 ... %d spans", who, span_count, RO_MAX_IQ_SPANS);
    if (!pending_count) return fail(RO_ERR_INVALID, "%s: null %spending_count", who, d);
    if (pending_capacity > 0 && !pending)
        return fail(RO_ERR_INVALID, "%s: null %spending with pending_capacity %lld", who, d, (long long)pending_capacity);
    if (!raw_dir || !raw_summary) return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, !raw_dir ? "raw_dir" : "raw_summary");
    if (arena_floats > 0 && !arena)
        return fail(RO_ERR_INVALID, "%s: null %sarena with arena_floats %lld", who, d, (long long)arena_floats);
    if (aligned && ((uintptr_t)arena & 7u) != 0) return fail(RO_ERR_INVALID, "%s: %sarena is not aligned to 8 bytes", who, d);
    for (int i = 0; i < span_count; ++i) {
        const ro_iq_span_t &s = spans[i];
        if (!s.d_iq) return fail(RO_ERR_INVALID, "%s: spans[%d]: null d_iq", who, i);
        if (s.format != RO_IQ_F32 && s.format != RO_IQ_I16 && s.format != RO_IQ_F64)
            return fail(RO_ERR_INVALID, "%s: spans[%d]: format %d is none of RO_IQ_F32, RO_IQ_I16, RO_IQ_F64", who, i, s.format);
        if (s.first_sample < 0 || s.samples < 1 || s.reserved != 0)
            return fail(RO_ERR_INVALID, "%s: spans[%d]: first_sample %lld, samples %lld, reserved %d: needs first_sample >= 0, "
                        "samples >= 1, reserved 0", who, i, (long long)s.first_sample, (long long)s.samples, s.reserved);
        if (aligned && ((uintptr_t)s.d_iq & (s.format == RO_IQ_I16 ? 3u : 7u)) != 0)
            return fail(RO_ERR_INVALID, "%s: spans[%d]: d_iq is not aligned to %d bytes", who, i, s.format == RO_IQ_I16 ? 4 : 8);
        if (i == 0) continue;
        const ro_iq_span_t &p = spans[i - 1];
        if (s.first_sample <= p.first_sample || s.first_sample + s.samples <= p.first_sample + p.samples)
            return fail(RO_ERR_INVALID, "%s: spans[%d] is out of order: [%lld, %lld) behind [%lld, %lld); first samples and ends "
                        "both ascend", who, i, (long long)s.first_sample, (long long)(s.first_sample + s.samples),
                        (long long)p.first_sample, (long long)(p.first_sample + p.samples));
        if (s.first_sample > p.first_sample + p.samples)
            return fail(RO_ERR_INVALID, "%s: spans[%d] leaves a gap: it begins at %lld, the one in front ends at %lld", who, i,
                        (long long)s.first_sample, (long long)(p.first_sample + p.samples));
    }
    if (dir_capacity > ro::RAW_MAX_CANDIDATES || pending_capacity > ro::RAW_MAX_CANDIDATES ||
        dir_capacity + pending_capacity > ro::RAW_MAX_CANDIDATES)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld + pending_capacity %lld: more than 2^24 candidates", who,
                    (long long)dir_capacity, (long long)pending_capacity);
    return RO_OK;
}

// (int)fft_sample_rate of the recorder's fftSamplesToRaw; 0 is the reference's division by zero
int raw_rate(const char *who, int sample_rate, int bins, int overlap, int *rate_r)
{
    *rate_r = (int)ro_fft_sample_rate(sample_rate, bins, overlap);
    if (*rate_r == 0)
        return fail(RO_ERR_UNSUPPORTED, "%s: %d samples/s over a hop of %d give an fft sample rate below 1: the raw length "
                    "divides by its integer part", who, sample_rate, bins - ro_clamp_overlap(bins, overlap));
    return RO_OK;
}

}  // namespace

extern "C" int ro_stft_raw_resident(ro_stft_t *h, const ro_snapshot_t *d_dir, int64_t dir_capacity,
                                    const ro_snap_summary_t *d_snap_summary, const ro_iq_span_t *spans, int span_count,
                                    ro_snapshot_t *d_pending, int64_t *d_pending_count, int64_t pending_capacity,
                                    ro_raw_capture_t *d_raw_dir, float *d_arena, int64_t arena_floats,
                                    ro_raw_summary_t *d_raw_summary, void *stream)
{
    const char *who = "ro_stft_raw_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int rc = raw_check(who, "d_", true, d_dir, dir_capacity, d_snap_summary, spans, span_count, d_pending, d_pending_count,
                       pending_capacity, d_raw_dir, d_arena, arena_floats, d_raw_summary);
    if (rc != RO_OK) return rc;
    int rate_r = 0;
    if ((rc = raw_rate(who, h->cfg.sample_rate, h->bins, h->cfg.overlap, &rate_r)) != RO_OK) return rc;
    int cus = 0;
    if ((rc = scratch_for(h, h->d_raw_scratch, ro::raw_scratch_bytes(dir_capacity, pending_capacity), &cus)) != RO_OK) return rc;
    ro::RawArgs a{};
    a.dir = d_dir;
    a.snap_summary = d_snap_summary;
    a.dir_capacity = dir_capacity;
    for (int i = 0; i < span_count; ++i) {
        a.iq[i] = spans[i].d_iq;
        a.first[i] = spans[i].first_sample;
        a.count[i] = spans[i].samples;
        a.format[i] = spans[i].format;
    }
    a.spans = span_count;
    a.base_sample = spans[0].first_sample;
    a.head_sample = spans[span_count - 1].first_sample + spans[span_count - 1].samples;
    a.hop = h->bins - ro_clamp_overlap(h->bins, h->cfg.overlap);
    a.z = ro_clamp_overlap(h->bins, h->cfg.overlap) == 0 ? 1 : 0;
    a.rate_r = (double)rate_r;
    a.sample_rate = (double)h->cfg.sample_rate;
    a.pending = d_pending;
    a.pending_count = d_pending_count;
    a.pending_capacity = pending_capacity;
    a.raw_dir = d_raw_dir;
    a.arena = d_arena;
    a.arena_floats = arena_floats;
    a.raw_summary = d_raw_summary;
    ro::raw_scratch_layout(a, h->d_raw_scratch);
    HIP_TRY(ro::launch_raw(a, cus, (hipStream_t)stream));
    return RO_OK;
}

// one sample of a span as the pair the reference stores (src/FFTBackend.h:250-254); RO_IQ_F32 moves bytes
static void raw_pair(const ro_iq_span_t &s, int64_t i, float *out)
{
    if (s.format == RO_IQ_F32) std::memcpy(out, static_cast<const char *>(s.d_iq) + 8 * i, 8);
    else if (s.format == RO_IQ_I16) {
        int16_t v[2];
        std::memcpy(v, static_cast<const char *>(s.d_iq) + 4 * i, 4);
        out[0] = (float)v[0];
        out[1] = (float)v[1];
    } else {
        double v[2];
        std::memcpy(v, static_cast<const char *>(s.d_iq) + 16 * i, 16);
        out[0] = (float)v[0];
        out[1] = (float)v[1];
    }
}

extern "C" int ro_raw_host(int bins, int overlap, int sample_rate, const ro_snapshot_t *dir, int64_t dir_capacity,
                           const ro_snap_summary_t *snap_summary, const ro_iq_span_t *spans, int span_count,
                           ro_snapshot_t *pending, int64_t *pending_count, int64_t pending_capacity,
                           ro_raw_capture_t *raw_dir, float *arena, int64_t arena_floats, ro_raw_summary_t *raw_summary)
{
    const char *who = "ro_raw_host";
    if (bins < 2) return fail(RO_ERR_INVALID, "%s: bins %d: at least 2", who, bins);
    int rc = raw_check(who, "", false, dir, dir_capacity, snap_summary, spans, span_count, pending, pending_count, pending_capacity,
                       raw_dir, arena, arena_floats, raw_summary);
    if (rc != RO_OK) return rc;
    int rate_r = 0;
    if ((rc = raw_rate(who, sample_rate, bins, overlap, &rate_r)) != RO_OK) return rc;
    const int64_t hop = bins - ro_clamp_overlap(bins, overlap), z = ro_clamp_overlap(bins, overlap) == 0 ? 1 : 0;
    const int64_t base = spans[0].first_sample, head = spans[span_count - 1].first_sample + spans[span_count - 1].samples;
    const int64_t have = std::min(std::max<int64_t>(*pending_count, 0), pending_capacity);
    const int64_t listed = std::min(std::max<int64_t>(snap_summary->resolved, 0), dir_capacity);
    ro_raw_summary_t sum{};
    int64_t offset = 0;                          // floats of every capturable candidate so far, fitting or not
    bool full = false;                           // one did not fit: nothing behind it does (the prefix only grows)
    int64_t still = 0;                           // candidates that stay pending; the first pending_capacity are kept
    for (int64_t c = 0; c < have + listed; ++c) {
        // (a kept candidate lands at or in front of the place it was read from: the list is compacted in place)
        const ro_snapshot_t e = c < have ? pending[c] : dir[c - have];
        if (c >= have && e.status != RO_SNAP_CAPTURED) continue;                 // no image, no raw run
        const int64_t start = e.event.start_row, len = (int64_t)e.rows + (e.first_row - start);
        const int64_t L = ro::raw_length(len, (double)rate_r, (double)sample_rate);
        const int64_t f = ro::raw_first_sample(start, hop, z);
        int status = -1;
        int64_t size = 0;
        if (f + L > head) status = -1;
        else if (L <= 0) status = RO_SNAP_EMPTY;
        else if (f < base) status = RO_SNAP_LOST;
        else {
            size = 2 * L;
            if (!full && size <= arena_floats - offset) status = RO_SNAP_CAPTURED;
            else full = true;
        }
        if (status < 0) {
            if (still < pending_capacity) pending[still] = e;
            still += 1;
        } else {
            ro_raw_capture_t &out = raw_dir[sum.resolved++];
            out.event = e.event;
            out.first_sample = f;
            out.samples = status == RO_SNAP_CAPTURED ? L : 0;
            out.offset = status == RO_SNAP_CAPTURED ? offset : 0;
            out.slot = e.slot;
            out.status = status;
            if (status == RO_SNAP_CAPTURED) {
                // the last span that holds a sample owns it: walk the run span by span, from the last one that begins at or
                // before the sample (no gap, ends ascending: it holds the sample)
                int i = span_count - 1;
                for (int64_t k = 0; k < L; ++k) {
                    const int64_t s = f + k;
                    while (i > 0 && spans[i].first_sample > s) --i;
                    while (i + 1 < span_count && spans[i + 1].first_sample <= s) ++i;
                    raw_pair(spans[i], s - spans[i].first_sample, arena + offset + 2 * k);
                }
                sum.captured += 1;
                sum.arena_floats = offset + size;
            } else if (status == RO_SNAP_EMPTY) sum.empty += 1;
            else sum.lost += 1;
        }
        if (!full) offset += size;
    }
    const int64_t kept = std::min(still, pending_capacity);
    *pending_count = kept;
    sum.pending = kept;
    sum.pending_dropped = still - kept;
    *raw_summary = sum;
    return RO_OK;
}
