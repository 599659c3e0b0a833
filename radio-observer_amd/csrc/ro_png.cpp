// ro_png.cpp -- the preview files (include/ro_stft.h; kernels: ro_png.hip): every level image of a level directory as a
// complete PNG in stored deflate blocks: argument checks, the handle's scratch, the launches; ro_levels_png_host, the same
// rules entry by entry over host memory with a byte-at-a-time CRC-32 and Adler-32; and ro_periodic_level_dir, a periodic
// plan's directory in level form.  Nothing in the resident call reads device memory.
#include "ro_host.h"

using namespace ro::host;

static_assert(RO_PNG_ALIGN == 16 && sizeof(ro_fits_unit_t) == 32, "the files' alignment and their directory are ABI");

int ro::host::png_check(const char *who, const char *d, bool aligned, const ro_fits_unit_t *level_dir, int64_t dir_capacity,
              const ro_unit_summary_t *level_summary, const void *levels, int64_t levels_bytes, const ro_fits_unit_t *png_dir,
              const void *png, int64_t png_bytes, const ro_unit_summary_t *png_summary)
{
    if (dir_capacity < 0 || levels_bytes < 0 || png_bytes < 0)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld, levels_bytes %lld, png_bytes %lld: none may be negative", who,
                    (long long)dir_capacity, (long long)levels_bytes, (long long)png_bytes);
    if (!level_summary) return fail(RO_ERR_INVALID, "%s: null %slevel_summary", who, d);
    if (dir_capacity > 0 && !level_dir)
        return fail(RO_ERR_INVALID, "%s: null %slevel_dir with dir_capacity %lld", who, d, (long long)dir_capacity);
    if (dir_capacity > ro::PNG_MAX_ENTRIES)
        return fail(RO_ERR_INVALID, "%s: dir_capacity %lld: more than 2^24 entries", who, (long long)dir_capacity);
    if (levels_bytes > 0 && !levels)
        return fail(RO_ERR_INVALID, "%s: null %slevels with levels_bytes %lld", who, d, (long long)levels_bytes);
    if (!png_dir || !png_summary) return fail(RO_ERR_INVALID, "%s: null %s%s", who, d, !png_dir ? "png_dir" : "png_summary");
    if (png_bytes > 0 && !png) return fail(RO_ERR_INVALID, "%s: null %spng with png_bytes %lld", who, d, (long long)png_bytes);
    if (aligned && ((uintptr_t)png & (RO_PNG_ALIGN - 1)) != 0)
        return fail(RO_ERR_INVALID, "%s: %spng is not aligned to 16 bytes", who, d);
    if (png_bytes > 0 && levels_bytes > 0) {
        const uintptr_t p = (uintptr_t)png, l = (uintptr_t)levels;
        if (p < l + (uintptr_t)levels_bytes && l < p + (uintptr_t)png_bytes)
            return fail(RO_ERR_INVALID, "%s: %spng overlaps %slevels: the files are written while the levels are read", who, d, d);
    }
    return RO_OK;
}

namespace {

constexpr ro::PngTables TABLES = ro::make_png_tables();

uint32_t crc_bytes(uint32_t c, const unsigned char *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) c = TABLES.byte[3][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

// one file on the host: the bytes in file order, then the two checksums over what was written
void write_png(const unsigned char *src, const ro::PngWant &w, unsigned char *file)
{
    int64_t raw, blocks, idat;
    ro::png_shape(w.naxis1, w.naxis2, &raw, &blocks, &idat);
    const unsigned len0 = (unsigned)std::min<int64_t>(raw, ro::PNG_STORED);
    for (int i = 12; i < 29; ++i) file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)w.naxis1, (uint32_t)w.naxis2, 0, 0, false, 0);
    const uint32_t ihdr_crc = ~crc_bytes(0xffffffffu, file + 12, 17);
    for (int i = 0; i < ro::PNG_DATA; ++i)
        file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)w.naxis1, (uint32_t)w.naxis2, ihdr_crc, (uint32_t)idat, blocks == 1, len0);
    uint32_t A = 1, B = 0;
    unsigned char *out = file + ro::PNG_HEAD;
    for (int64_t i = 0; i < raw; ++i) {
        if (i % ro::PNG_STORED == 0) {
            const unsigned len = (unsigned)std::min<int64_t>(raw - i, ro::PNG_STORED);
            for (int j = 0; j < 5; ++j) *out++ = (unsigned char)ro::png_block_header_byte(j, raw - i <= ro::PNG_STORED, len);
        }
        const int64_t row = i / (w.naxis1 + (int64_t)1), col = i % (w.naxis1 + (int64_t)1);
        const unsigned char v = col == 0 ? 0 : src[row * w.naxis1 + col - 1];
        *out++ = v;
        A = (A + v) % ro::ADLER_MOD;
        B = (B + A) % ro::ADLER_MOD;
    }
    const uint32_t adler = (B << 16) | A;
    for (int i = 0; i < 4; ++i) out[i] = (unsigned char)ro::png_tail_byte(i, adler, 0);
    const uint32_t crc = ~crc_bytes(0xffffffffu, file + 37, 4 + idat);
    for (int i = 4; i < ro::PNG_TAIL; ++i) out[i] = (unsigned char)ro::png_tail_byte(i, adler, crc);
    std::memset(out + ro::PNG_TAIL, 0, (size_t)(ro::png_room(w.bytes) - w.bytes));
}

}  // namespace

extern "C" int64_t ro_png_bytes(int32_t naxis1, int64_t naxis2)
{
    const int64_t bytes = ro::png_file_bytes(naxis1, naxis2);
    if (bytes < 0)
        return fail(RO_ERR_INVALID, "ro_png_bytes: naxis1 %d, naxis2 %lld: at least 1 x 1, and an IDAT of at most 2^31 - 1 bytes",
                    naxis1, (long long)naxis2);
    return bytes;
}

extern "C" int ro_stft_levels_png_resident(ro_stft_t *h, const ro_fits_unit_t *d_level_dir, int64_t dir_capacity,
                                           const ro_unit_summary_t *d_level_summary, const void *d_levels, int64_t levels_bytes,
                                           ro_fits_unit_t *d_png_dir, void *d_png, int64_t png_bytes,
                                           ro_unit_summary_t *d_png_summary, void *stream)
{
    const char *who = "ro_stft_levels_png_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int rc = png_check(who, "d_", true, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png, png_bytes,
                       d_png_summary);
    if (rc != RO_OK) return rc;
    ro::PngArgs a{};
    a.level_dir = d_level_dir;
    a.entries = &d_level_summary->entries;
    a.dir_capacity = dir_capacity;
    a.levels = static_cast<const unsigned char *>(d_levels);
    a.levels_bytes = levels_bytes;
    a.png_dir = d_png_dir;
    a.png = static_cast<char *>(d_png);
    a.png_bytes = png_bytes;
    a.summary = d_png_summary;
    HIP_TRY(hipSetDevice(h->device));
    int cus = 0;
    if ((rc = device_cus(h, &cus)) != RO_OK) return rc;
    if ((rc = grow_scratch(h->d_png_scratch, ro::png_scratch_bytes(dir_capacity, png_bytes))) != RO_OK) return rc;
    ro::png_scratch_layout(a, h->d_png_scratch);
    HIP_TRY(ro::launch_levels_png(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_levels_png_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                                  const void *levels, int64_t levels_bytes, ro_fits_unit_t *png_dir, void *png, int64_t png_bytes,
                                  ro_unit_summary_t *png_summary)
{
    const char *who = "ro_levels_png_host";
    const int rc = png_check(who, "", false, level_dir, dir_capacity, level_summary, levels, levels_bytes, png_dir, png, png_bytes,
                             png_summary);
    if (rc != RO_OK) return rc;
    const int64_t n = entries_of(level_summary->entries, dir_capacity);
    ro_unit_summary_t sum{};
    sum.entries = n;
    int64_t first = 0;                           // rooms of every writable entry so far, fitting or not
    for (int64_t d = 0; d < n; ++d) {
        const ro_fits_unit_t &e = level_dir[d];
        const ro::PngWant w = ro::png_want(e.offset, e.bytes, e.naxis2, e.naxis1, e.status, levels_bytes);
        ro_fits_unit_t out{};
        out.status = w.status;
        if (w.status == RO_UNIT_SKIPPED) sum.skipped += 1;
        else if (w.status == RO_UNIT_INVALID) sum.invalid += 1;
        else {
            const int64_t room = ro::png_room(w.bytes);
            out.bytes = w.bytes;
            out.naxis2 = w.naxis2;
            out.naxis1 = w.naxis1;
            if (first + room <= png_bytes) {
                out.offset = first;
                write_png(static_cast<const unsigned char *>(levels) + w.source, w, static_cast<unsigned char *>(png) + first);
                sum.written += 1;
                sum.units_bytes = first + room;
            } else {
                out.status = RO_UNIT_NO_ROOM;
                sum.no_room += 1;
            }
            first += room;
        }
        png_dir[d] = out;
    }
    sum.needed_bytes = first;
    *png_summary = sum;
    return RO_OK;
}

extern "C" int ro_periodic_level_dir(const ro_periodic_entry_t *dir, int64_t entries, ro_fits_unit_t *level_dir,
                                     ro_unit_summary_t *level_summary)
{
    const char *who = "ro_periodic_level_dir";
    if (entries < 0) return fail(RO_ERR_INVALID, "%s: entries %lld: may not be negative", who, (long long)entries);
    if (entries > 0 && (!dir || !level_dir)) return fail(RO_ERR_INVALID, "%s: null %s with entries %lld", who, !dir ? "dir" : "level_dir", (long long)entries);
    if (!level_summary) return fail(RO_ERR_INVALID, "%s: null level_summary", who);
    for (int64_t d = 0; d < entries; ++d)
        if (dir[d].status != RO_PERIODIC_WRITTEN && dir[d].status != RO_PERIODIC_LOST && dir[d].status != RO_PERIODIC_NO_ROOM)
            return fail(RO_ERR_INVALID, "%s: dir[%lld].status %d: not a status of ro_periodic_plan", who, (long long)d, dir[d].status);
    ro_unit_summary_t sum{};
    sum.entries = entries;
    for (int64_t d = 0; d < entries; ++d) {
        const ro_periodic_entry_t &e = dir[d];
        ro_fits_unit_t out{};
        out.status = RO_UNIT_SKIPPED;
        if (e.status == RO_PERIODIC_WRITTEN) {
            out.offset = e.offset / 4;
            out.bytes = (int64_t)e.naxis1 * e.rows;
            out.naxis2 = e.rows;
            out.naxis1 = e.naxis1;
            out.status = RO_UNIT_WRITTEN;
            sum.written += 1;
            sum.units_bytes = std::max(sum.units_bytes, (e.offset + ro::periodic_blocks(e.naxis1, e.rows) * RO_FITS_BLOCK) / 4);
        } else sum.skipped += 1;
        level_dir[d] = out;
    }
    sum.needed_bytes = sum.units_bytes;
    *level_summary = sum;
    return RO_OK;
}
