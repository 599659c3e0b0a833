// ro_png.cpp -- the preview files (include/ro_stft.h; kernels: ro_png.hip): every level image of a level directory as a
// complete PNG in stored deflate blocks: argument checks, the handle's scratch, the launches; the host's one file writer (the
// raw bytes block by block, a byte-at-a-time CRC-32 and Adler-32, the frame around the blocks) and the host twins of both
// kinds of file over it -- ro_levels_png_host with every block stored, ro_levels_png_deflate_host with the blocks' codes of
// ro_png_deflate.cpp -- each pack_walk over its own entry rule; and ro_periodic_level_dir, a periodic plan's directory in
// level form.  Nothing in the resident call reads device memory.
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

void ro::host::png_fill_args(ro::PngArgs &a, const ro_fits_unit_t *level_dir, int64_t dir_capacity,
                             const ro_unit_summary_t *level_summary, const void *levels, int64_t levels_bytes,
                             ro_fits_unit_t *png_dir, void *png, int64_t png_bytes, ro_unit_summary_t *png_summary)
{
    a.level_dir = level_dir;
    a.entries = &level_summary->entries;
    a.dir_capacity = dir_capacity;
    a.levels = static_cast<const unsigned char *>(levels);
    a.levels_bytes = levels_bytes;
    a.png_dir = png_dir;
    a.png = static_cast<char *>(png);
    a.png_bytes = png_bytes;
    a.summary = png_summary;
}

namespace {

constexpr ro::PngTables TABLES = ro::make_png_tables();

uint32_t crc_bytes(uint32_t c, const unsigned char *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) c = TABLES.byte[3][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

// the raw bytes of an image of scanlines of naxis1 levels -- a filter byte 0 in front of every scanline -- in blocks of
// PNG_STORED: fn(the block's raw bytes, how many, whether it is the last)
template <class Fn> void each_block(const unsigned char *src, int64_t naxis1, int64_t raw, Fn fn)
{
    std::vector<unsigned char> part((size_t)std::min<int64_t>(raw, ro::PNG_STORED));
    int64_t col = 0;                             // of the next raw byte in its scanline; 0: the filter byte
    for (int64_t r0 = 0; r0 < raw; r0 += ro::PNG_STORED) {
        const int64_t len = std::min<int64_t>(raw - r0, ro::PNG_STORED);
        for (int64_t i = 0; i < len; ++i) {
            part[(size_t)i] = col == 0 ? 0 : *src++;
            col = col == naxis1 ? 0 : col + 1;
        }
        fn(part.data(), len, r0 + len == raw);
    }
}

// One file on the host: the blocks in file order -- block k in the form of codes[k], every block stored where codes is null
// -- then the frame around them: IHDR with its CRC and the rest of the 43-byte head, the Adler-32, the IDAT CRC, IEND.  The
// zeros up to the file's room are the walk's
void write_png(const unsigned char *src, int32_t naxis1, int64_t naxis2, const DeflateCode *codes, unsigned char *file)
{
    int64_t stream = 0;
    uint32_t A = 1, B = 0;
    each_block(src, naxis1, naxis2 * ((int64_t)naxis1 + 1), [&](const unsigned char *raw, int64_t len, bool last) {
        stream += deflate_write_block(raw, len, last, codes ? codes++ : nullptr, file + ro::PNG_HEAD + stream);
        // (5552 bytes are zlib's NMAX: the most whose sums, from remainders, stay below 2^32 without the modulus)
        for (int64_t i = 0; i < len;) {
            for (const int64_t end = std::min<int64_t>(len, i + 5552); i < end; ++i) {
                A += raw[i];
                B += A;
            }
            A %= ro::ADLER_MOD;
            B %= ro::ADLER_MOD;
        }
    });
    const uint32_t adler = (B << 16) | A;
    const int64_t idat = ro::deflate_idat(stream);
    for (int i = 12; i < 29; ++i) file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)naxis1, (uint32_t)naxis2, 0, 0, false, 0);
    const uint32_t ihdr_crc = ~crc_bytes(0xffffffffu, file + 12, 17);
    for (int i = 0; i < ro::PNG_HEAD; ++i)
        file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)naxis1, (uint32_t)naxis2, ihdr_crc, (uint32_t)idat, false, 0);
    unsigned char *tail = file + ro::PNG_HEAD + stream;
    for (int i = 0; i < 4; ++i) tail[i] = (unsigned char)ro::png_tail_byte(i, adler, 0);
    const uint32_t crc = ~crc_bytes(0xffffffffu, file + 37, 4 + idat);
    for (int i = 4; i < ro::PNG_TAIL; ++i) tail[i] = (unsigned char)ro::png_tail_byte(i, adler, crc);
}

ro::PngWant want_of(const ro_fits_unit_t &e, int64_t levels_bytes)
{
    return ro::png_want(e.offset, e.bytes, e.naxis2, e.naxis1, e.status, levels_bytes);
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
    png_fill_args(a, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png, png_bytes, d_png_summary);
    int cus = 0;
    if ((rc = scratch_for(h, h->d_png_scratch, ro::png_scratch_bytes(dir_capacity, png_bytes), &cus)) != RO_OK) return rc;
    ro::png_scratch_layout(a, h->d_png_scratch);
    HIP_TRY(ro::launch_levels_png(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_levels_png_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity, const ro_unit_summary_t *level_summary,
                                  const void *levels, int64_t levels_bytes, ro_fits_unit_t *png_dir, void *png, int64_t png_bytes,
                                  ro_unit_summary_t *png_summary)
{
    const int rc = png_check("ro_levels_png_host", "", false, level_dir, dir_capacity, level_summary, levels, levels_bytes, png_dir, png,
                             png_bytes, png_summary);
    if (rc != RO_OK) return rc;
    // a file's size is arithmetic on its shape
    pack_walk(entries_of(level_summary->entries, dir_capacity), [&](int64_t d) {
        const ro::PngWant w = want_of(level_dir[d], levels_bytes);
        return WalkWant{w.status, w.naxis1, w.naxis2, w.bytes, ro::png_room(w.bytes)};
    }, [&](int64_t d, unsigned char *dst) {
        const ro_fits_unit_t &e = level_dir[d];
        write_png(static_cast<const unsigned char *>(levels) + e.offset, e.naxis1, e.naxis2, nullptr, dst);
    }, png_dir, png, png_bytes, png_summary);
    return RO_OK;
}

extern "C" int ro_levels_png_deflate_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity,
                                          const ro_unit_summary_t *level_summary, const void *levels, int64_t levels_bytes,
                                          ro_fits_unit_t *png_dir, void *png, int64_t png_bytes, ro_unit_summary_t *png_summary)
{
    const int rc = png_check("ro_levels_png_deflate_host", "", false, level_dir, dir_capacity, level_summary, levels, levels_bytes,
                             png_dir, png, png_bytes, png_summary);
    if (rc != RO_OK) return rc;
    const int64_t max_blocks = ro::deflate_max_blocks(dir_capacity, levels_bytes);
    int64_t blocks = 0;                          // blocks of every entry rule 2 passes so far
    std::vector<DeflateCode> codes;              // the blocks' codes of the entry the walk is at: want measures, emit writes
    // a file's size is its data's: the entry is measured block by block, unless its blocks pass the bound of the device's
    // scratch (images that overlap each other)
    pack_walk(entries_of(level_summary->entries, dir_capacity), [&](int64_t d) {
        const ro::PngWant w = want_of(level_dir[d], levels_bytes);
        if (w.status != RO_UNIT_WRITTEN) return WalkWant{w.status, 0, 0, 0, 0};
        blocks += w.blocks;
        if (blocks > max_blocks) return WalkWant{RO_UNIT_INVALID, 0, 0, 0, 0};
        codes.clear();
        int64_t stream = 0;
        each_block(static_cast<const unsigned char *>(levels) + w.source, w.naxis1, w.naxis2 * ((int64_t)w.naxis1 + 1),
                   [&](const unsigned char *raw, int64_t len, bool last) {
                       codes.push_back(deflate_code(raw, len, last));
                       stream += codes.back().bytes;
                   });
        const int64_t bytes = ro::deflate_file_bytes(stream);
        return WalkWant{RO_UNIT_WRITTEN, w.naxis1, w.naxis2, bytes, ro::png_room(bytes)};
    }, [&](int64_t d, unsigned char *dst) {
        const ro_fits_unit_t &e = level_dir[d];
        write_png(static_cast<const unsigned char *>(levels) + e.offset, e.naxis1, e.naxis2, codes.data(), dst);
    }, png_dir, png, png_bytes, png_summary);
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
