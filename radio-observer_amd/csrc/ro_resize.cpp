// ro_resize.cpp -- resized previews (include/ro_stft.h; kernels: ro_resize.hip; the plan blob: ro_resize.h): fits2png's
// --width.  The plan is host arithmetic: ro_resize_shape, and ro_resize_plan, which walks a HOST level directory by the
// family's entry rules, writes the out directory and summary, and builds the jobs and the tap tables -- Pillow's
// precompute_coeffs and normalize_coeffs_8bpc for the Lanczos filter, in double with the C library's sin, one table per
// distinct (in, out) pair.  ro_stft_levels_resize_resident checks its arguments, grows the handle's scratch for the
// intermediate images and launches; ro_levels_resize_host runs the same jobs over host memory with the same checks, bounds
// and int32 sums, so equal inputs give equal bytes.
#include "ro_host.h"

#include <map>
#include <utility>

using namespace ro::host;

static_assert(sizeof(ro_resize_info_t) == 64, "the info struct is ABI");

namespace {

double sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}

double lanczos(double x) { return -3.0 <= x && x < 3.0 ? sinc(x) * sinc(x / 3) : 0.0; }

// rows of a table: ksize = (int)ceil(support) * 2 + 1, but no more than `in`, which no xmax passes
int64_t table_ksize(int32_t in, int32_t out)
{
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale;
    const int64_t ksize = (int64_t)std::ceil(3.0 * fs) * 2 + 1;
    return std::min<int64_t>(ksize, in);
}

// the table of (in, out) at `at`: every product and sum below is one rounding, in the order written
void build_table(int32_t in, int32_t out, char *at)
{
#pragma clang fp contract(off)
    const int64_t ksize = table_ksize(in, out);
    ro::ResizeTableHead head = {in, out, (int32_t)ksize, 0};
    std::memcpy(at, &head, sizeof head);
    int32_t *bounds = reinterpret_cast<int32_t *>(at + sizeof head), *taps = bounds + 2 * (int64_t)out;
    const double scale = (double)in / (double)out, fs = scale < 1.0 ? 1.0 : scale, support = 3.0 * fs, ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int32_t xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int64_t xmin = (int64_t)(center - support + 0.5), xmax = (int64_t)(center + support + 0.5);
        xmin = std::max<int64_t>(xmin, 0);
        xmax = std::min<int64_t>(xmax, in) - xmin;
        xmax = std::min(std::max<int64_t>(xmax, 0), ksize);
        double ww = 0.0;
        for (int64_t x = 0; x < xmax; ++x) {
            w[(size_t)x] = lanczos((x + xmin - center + 0.5) * ss);
            ww += w[(size_t)x];
        }
        for (int64_t x = 0; x < ksize; ++x) {
            double k = x < xmax ? w[(size_t)x] : 0.0;
            if (x < xmax && ww != 0.0) k /= ww;
            taps[x * out + xx] = k < 0 ? (int32_t)(-0.5 + k * (double)(1 << ro::RESIZE_BITS)) : (int32_t)(0.5 + k * (double)(1 << ro::RESIZE_BITS));
        }
        bounds[2 * (int64_t)xx] = (int32_t)xmin;
        bounds[2 * (int64_t)xx + 1] = (int32_t)xmax;
    }
}

void shape_of(int32_t naxis1, int64_t naxis2, int32_t width, int32_t *out_naxis1, int64_t *out_naxis2)
{
    *out_naxis1 = naxis1;
    *out_naxis2 = naxis2;
    if (width < naxis1) {
        const double ratio = (double)width / (double)naxis1;
        *out_naxis1 = width;
        *out_naxis2 = (int64_t)((double)naxis2 * ratio);
    }
}

// the horizontal pass over host memory: `rows` rows of t.in pixels to rows of t.out, row by row; every pixel's taps are
// gathered once, side by side (the table has them a column apart)
void pass_rows(const ro::ResizeTable &t, const unsigned char *in, int64_t rows, unsigned char *out)
{
    std::vector<int32_t> k((size_t)t.ksize * (size_t)t.out), lo((size_t)t.out), n((size_t)t.out);
    for (int32_t xx = 0; xx < t.out; ++xx) {
        ro::resize_bounds(t, xx, lo[(size_t)xx], n[(size_t)xx]);
        for (int32_t x = 0; x < n[(size_t)xx]; ++x) k[(size_t)xx * (size_t)t.ksize + (size_t)x] = t.taps[(int64_t)x * t.out + xx];
    }
    for (int64_t r = 0; r < rows; ++r)
        for (int32_t xx = 0; xx < t.out; ++xx) {
            int32_t sum = 1 << (ro::RESIZE_BITS - 1);
            const unsigned char *p = in + r * t.in + lo[(size_t)xx];
            const int32_t *kk = &k[(size_t)xx * (size_t)t.ksize];
            for (int32_t x = 0; x < n[(size_t)xx]; ++x) sum += (int32_t)p[x] * kk[x];
            out[r * t.out + xx] = ro::resize_clip(sum);
        }
}

// the vertical pass: t.in rows of `cols` pixels to t.out rows, a row of sums at a time, so that every tap reads one input row
void pass_cols(const ro::ResizeTable &t, const unsigned char *in, int64_t cols, unsigned char *out)
{
    std::vector<int32_t> sum((size_t)cols);
    for (int32_t yy = 0; yy < t.out; ++yy) {
        int32_t lo, n;
        ro::resize_bounds(t, yy, lo, n);
        std::fill(sum.begin(), sum.end(), 1 << (ro::RESIZE_BITS - 1));
        for (int32_t x = 0; x < n; ++x) {
            const int32_t k = t.taps[(int64_t)x * t.out + yy];
            const unsigned char *p = in + (int64_t)(lo + x) * cols;
            for (int64_t c = 0; c < cols; ++c) sum[(size_t)c] += (int32_t)p[c] * k;
        }
        for (int64_t c = 0; c < cols; ++c) out[(int64_t)yy * cols + c] = ro::resize_clip(sum[(size_t)c]);
    }
}

int info_check(const char *who, const ro_resize_info_t *info)
{
    if (!info) return fail(RO_ERR_INVALID, "%s: null info", who);
    if (info->jobs < 0 || info->h_items < 0 || info->v_items < 0 || info->mid_bytes < 0 || info->plan_bytes < (int64_t)sizeof(ro::ResizePlanHead))
        return fail(RO_ERR_INVALID, "%s: info is not what ro_resize_plan writes (jobs %lld, items %lld and %lld, mid_bytes %lld, plan_bytes %lld)",
                    who, (long long)info->jobs, (long long)info->h_items, (long long)info->v_items, (long long)info->mid_bytes,
                    (long long)info->plan_bytes);
    return RO_OK;
}

bool overlaps(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes)
{
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return a_bytes > 0 && b_bytes > 0 && p < q + (uintptr_t)b_bytes && q < p + (uintptr_t)a_bytes;
}

// what the two resize calls ask of their buffers, as a refusal in the name of `who`
int buffers_check(const char *who, const char *d, int align, const void *plan, int64_t plan_bytes, const void *levels, int64_t levels_bytes,
                  const void *out_levels, int64_t out_levels_bytes)
{
    if (levels_bytes < 0 || out_levels_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: levels_bytes %lld, out_levels_bytes %lld: none may be negative", who, (long long)levels_bytes,
                    (long long)out_levels_bytes);
    if (!plan) return fail(RO_ERR_INVALID, "%s: null %splan", who, d);
    if (levels_bytes > 0 && !levels) return fail(RO_ERR_INVALID, "%s: null %slevels with levels_bytes %lld", who, d, (long long)levels_bytes);
    if (out_levels_bytes > 0 && !out_levels)
        return fail(RO_ERR_INVALID, "%s: null %sout_levels with out_levels_bytes %lld", who, d, (long long)out_levels_bytes);
    if (((uintptr_t)plan & (uintptr_t)(align - 1)) != 0) return fail(RO_ERR_INVALID, "%s: %splan is not aligned to %d bytes", who, d, align);
    if (align > 8 && ((uintptr_t)levels & (uintptr_t)(align - 1)) != 0)
        return fail(RO_ERR_INVALID, "%s: %slevels is not aligned to %d bytes", who, d, align);
    if (align > 8 && ((uintptr_t)out_levels & (uintptr_t)(align - 1)) != 0)
        return fail(RO_ERR_INVALID, "%s: %sout_levels is not aligned to %d bytes", who, d, align);
    if (overlaps(out_levels, out_levels_bytes, levels, levels_bytes))
        return fail(RO_ERR_INVALID, "%s: %sout_levels overlaps %slevels: the images are written while the levels are read", who, d, d);
    if (overlaps(out_levels, out_levels_bytes, plan, plan_bytes))
        return fail(RO_ERR_INVALID, "%s: %sout_levels overlaps %splan: the images are written while the plan is read", who, d, d);
    return RO_OK;
}

}  // namespace

extern "C" int ro_resize_shape(int32_t naxis1, int64_t naxis2, int32_t width, int32_t *out_naxis1, int64_t *out_naxis2)
{
    if (naxis1 < 1 || naxis2 < 1 || width < 1)
        return fail(RO_ERR_INVALID, "ro_resize_shape: naxis1 %d, naxis2 %lld, width %d: each at least 1", naxis1, (long long)naxis2, width);
    if (!out_naxis1 || !out_naxis2) return fail(RO_ERR_INVALID, "ro_resize_shape: null %s", !out_naxis1 ? "out_naxis1" : "out_naxis2");
    shape_of(naxis1, naxis2, width, out_naxis1, out_naxis2);
    return RO_OK;
}

extern "C" int ro_resize_plan(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                              int64_t levels_bytes, int32_t width, ro_fits_unit_t *out_level_dir, int64_t out_levels_bytes,
                              ro_unit_summary_t *out_level_summary, void *plan, int64_t plan_bytes, ro_resize_info_t *info)
{
    const char *who = "ro_resize_plan";
    if (dir_capacity < 0 || levels_bytes < 0 || out_levels_bytes < 0 || plan_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld, levels_bytes %lld, out_levels_bytes %lld, plan_bytes %lld: none may be negative", who,
                    (long long)dir_capacity, (long long)levels_bytes, (long long)out_levels_bytes, (long long)plan_bytes);
    if (width < 1) return fail(RO_ERR_INVALID, "%s: width %d: at least 1", who, width);
    if (!level_summary) return fail(RO_ERR_INVALID, "%s: null level_summary", who);
    if (dir_capacity > 0 && !level_dir) return fail(RO_ERR_INVALID, "%s: null level_dir with dir_capacity %lld", who, (long long)dir_capacity);
    if (dir_capacity > ro::PNG_MAX_ENTRIES) return fail(RO_ERR_INVALID, "%s: dir_capacity %lld: more than 2^24 entries", who, (long long)dir_capacity);
    if (!out_level_dir || !out_level_summary)
        return fail(RO_ERR_INVALID, "%s: null %s", who, !out_level_dir ? "out_level_dir" : "out_level_summary");
    if (!info) return fail(RO_ERR_INVALID, "%s: null info", who);
    if (!plan && plan_bytes > 0) return fail(RO_ERR_INVALID, "%s: null plan with plan_bytes %lld", who, (long long)plan_bytes);
    if (plan && ((uintptr_t)plan & 7u) != 0) return fail(RO_ERR_INVALID, "%s: plan is not aligned to 8 bytes", who);

    // the directory, by the family's walk (pack_walk, without a buffer to write)
    const int64_t n = entries_of(level_summary->entries, dir_capacity);
    ro_unit_summary_t sum{};
    sum.entries = n;
    std::vector<ro::ResizeJob> jobs;
    int64_t first = 0, h_items = 0, v_items = 0, mid_bytes = 0;
    for (int64_t d = 0; d < n; ++d) {
        const ro_fits_unit_t &e = level_dir[d];
        const ro::PngWant w = ro::png_want(e.offset, e.bytes, e.naxis2, e.naxis1, e.status, levels_bytes);
        ro_fits_unit_t out{};
        out.status = w.status;
        int32_t w_out = 0;
        int64_t h_out = 0;
        if (w.status == RO_UNIT_WRITTEN) {
            shape_of(w.naxis1, w.naxis2, width, &w_out, &h_out);
            if (h_out == 0) out.status = RO_UNIT_SKIPPED;            // fits2png has no image to save
        }
        if (out.status == RO_UNIT_SKIPPED) sum.skipped += 1;
        else if (out.status == RO_UNIT_INVALID) sum.invalid += 1;
        else {
            out.bytes = (int64_t)w_out * h_out;
            out.naxis2 = h_out;
            out.naxis1 = w_out;
            const int64_t room = ro::resize_up(out.bytes, RO_LEVEL_BLOCK);
            if (first + room <= out_levels_bytes) {
                out.offset = first;
                ro::ResizeJob j{};
                j.src = w.source;
                j.dst = first;
                j.w = w.naxis1;
                j.h = (int32_t)w.naxis2;
                j.w_out = w_out;
                j.h_out = (int32_t)h_out;
                j.first_h = h_items;
                j.first_v = v_items;
                // (width < w makes h_out < h too: both passes, or a copy)
                const bool resized = j.w != j.w_out;
                if (resized) h_items += ro::resize_h_items(j.w_out, j.h);
                v_items += 1 + (resized ? ro::resize_v_items(j.w_out, j.h_out) : ro::resize_copy_items(out.bytes));
                if (resized) {
                    j.mid = mid_bytes;
                    mid_bytes += ro::resize_up((int64_t)j.w_out * j.h, ro::RESIZE_ALIGN);
                }
                jobs.push_back(j);
                sum.written += 1;
                sum.units_bytes = first + room;
            } else {
                out.status = RO_UNIT_NO_ROOM;
                sum.no_room += 1;
            }
            first += room;
        }
        out_level_dir[d] = out;
    }
    sum.needed_bytes = first;
    *out_level_summary = sum;

    // where the tables go: one per distinct (in, out), in the order the jobs ask for them
    std::map<std::pair<int32_t, int32_t>, int64_t> tables;
    int64_t need = ro::resize_up((int64_t)sizeof(ro::ResizePlanHead) + (int64_t)jobs.size() * (int64_t)sizeof(ro::ResizeJob), ro::RESIZE_ALIGN);
    auto table_at = [&](int32_t in, int32_t out) -> int64_t {
        if (in == out) return 0;
        const auto key = std::make_pair(in, out);
        const auto it = tables.find(key);
        if (it != tables.end()) return it->second;
        const int64_t at = need;
        tables.emplace(key, at);
        need += ro::resize_table_bytes(out, table_ksize(in, out));
        return at;
    };
    for (ro::ResizeJob &j : jobs) {
        j.table_h = table_at(j.w, j.w_out);
        j.table_v = table_at(j.h, j.h_out);
    }
    ro_resize_info_t inf{};
    inf.jobs = (int64_t)jobs.size();
    inf.h_items = h_items;
    inf.v_items = v_items;
    inf.mid_bytes = mid_bytes;
    inf.plan_bytes = need;
    *info = inf;
    if (!plan && plan_bytes == 0) return RO_OK;  // the sizing form
    if (plan_bytes < need)
        return fail(RO_ERR_INVALID, "%s: plan_bytes %lld: the plan takes %lld (info->plan_bytes)", who, (long long)plan_bytes, (long long)need);
    char *blob = static_cast<char *>(plan);
    std::memset(blob, 0, (size_t)need);
    ro::ResizePlanHead head{};
    head.magic = ro::RESIZE_MAGIC;
    head.jobs = inf.jobs;
    head.h_items = h_items;
    head.v_items = v_items;
    head.mid_bytes = mid_bytes;
    head.plan_bytes = need;
    std::memcpy(blob, &head, sizeof head);
    if (!jobs.empty()) std::memcpy(blob + sizeof head, jobs.data(), jobs.size() * sizeof(ro::ResizeJob));
    for (const auto &t : tables) build_table(t.first.first, t.first.second, blob + t.second);
    return RO_OK;
}

extern "C" int ro_stft_levels_resize_resident(ro_stft_t *h, const ro_resize_info_t *info, const void *d_plan, const void *d_levels,
                                              int64_t levels_bytes, void *d_out_levels, int64_t out_levels_bytes, void *stream)
{
    const char *who = "ro_stft_levels_resize_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int rc = info_check(who, info);
    if (rc != RO_OK) return rc;
    if ((rc = buffers_check(who, "d_", ro::RESIZE_ALIGN, d_plan, info->plan_bytes, d_levels, levels_bytes, d_out_levels, out_levels_bytes)) != RO_OK)
        return rc;
    if (info->jobs == 0) return RO_OK;
    int cus = 0;
    if ((rc = scratch_for(h, h->d_resize_scratch, (size_t)std::max<int64_t>(info->mid_bytes, ro::RESIZE_ALIGN), &cus)) != RO_OK) return rc;
    ro::ResizeArgs a{};
    a.plan = static_cast<const char *>(d_plan);
    a.plan_bytes = info->plan_bytes;
    a.levels = static_cast<const unsigned char *>(d_levels);
    a.levels_bytes = levels_bytes;
    a.out_levels = static_cast<unsigned char *>(d_out_levels);
    a.out_levels_bytes = out_levels_bytes;
    a.mid = reinterpret_cast<unsigned char *>(static_cast<char *>(h->d_resize_scratch));
    a.mid_bytes = info->mid_bytes;
    a.h_items = info->h_items;
    a.v_items = info->v_items;
    HIP_TRY(ro::launch_levels_resize(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_levels_resize_host(const ro_resize_info_t *info, const void *plan, const void *levels, int64_t levels_bytes,
                                     void *out_levels, int64_t out_levels_bytes)
{
    const char *who = "ro_levels_resize_host";
    int rc = info_check(who, info);
    if (rc != RO_OK) return rc;
    if ((rc = buffers_check(who, "", 8, plan, info->plan_bytes, levels, levels_bytes, out_levels, out_levels_bytes)) != RO_OK) return rc;
    const char *blob = static_cast<const char *>(plan);
    if (!ro::resize_head_ok(blob, info->plan_bytes))
        return fail(RO_ERR_INVALID, "%s: plan is not the plan of info->plan_bytes %lld bytes ro_resize_plan wrote", who, (long long)info->plan_bytes);
    const ro::ResizePlanHead *head = reinterpret_cast<const ro::ResizePlanHead *>(blob);
    const ro::ResizeJob *jobs = reinterpret_cast<const ro::ResizeJob *>(blob + sizeof(ro::ResizePlanHead));
    const unsigned char *src = static_cast<const unsigned char *>(levels);
    unsigned char *dst = static_cast<unsigned char *>(out_levels);
    std::vector<unsigned char> mid;
    for (int64_t d = 0; d < head->jobs; ++d) {
        const ro::ResizeJob &j = jobs[d];
        // (the intermediate image is this loop's own, but a job has to fit the room the device call would give it)
        const ro::ResizeRooms rooms = {levels_bytes, out_levels_bytes, info->mid_bytes, info->plan_bytes};
        ro::ResizeTable th{}, tv{};
        if (!ro::resize_job_ok(blob, rooms, j, th, tv)) continue;
        const bool resized = j.w != j.w_out;
        const int64_t out_bytes = (int64_t)j.w_out * j.h_out;
        const unsigned char *in = src + j.src;
        unsigned char *out = dst + j.dst;
        if (resized) mid.resize((size_t)((int64_t)j.w_out * j.h));
        if (resized) {
            pass_rows(th, in, j.h, mid.data());
            pass_cols(tv, mid.data(), j.w_out, out);
        } else std::memcpy(out, in, (size_t)out_bytes);
        std::memset(out + out_bytes, 0, (size_t)(ro::resize_up(out_bytes, RO_LEVEL_BLOCK) - out_bytes));
    }
    return RO_OK;
}
