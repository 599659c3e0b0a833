// ro_png_deflate.cpp -- the compressed preview files (include/ro_stft.h; kernels: ro_png_deflate.hip): every level image of a
// level directory as a complete PNG whose deflate blocks are Huffman coded where that is shorter: argument checks, the
// handle's scratch, the launches; and ro_levels_png_deflate_host, the same rules entry by entry and block by block over host
// memory with a bit writer and a byte-at-a-time CRC-32 and Adler-32.  Nothing in the resident call reads device memory.
#include "ro_host.h"

using namespace ro::host;

namespace {

constexpr ro::PngTables TABLES = ro::make_png_tables();

uint32_t crc_bytes(uint32_t c, const unsigned char *p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) c = TABLES.byte[3][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

// raw bytes [r0, r0 + len) of an image of scanlines of naxis1 levels: a filter byte 0 in front of every scanline
void raw_bytes(const unsigned char *src, int64_t naxis1, int64_t r0, int64_t len, unsigned char *raw)
{
    for (int64_t i = 0; i < len; ++i) {
        const int64_t row = (r0 + i) / (naxis1 + 1), col = (r0 + i) % (naxis1 + 1);
        raw[i] = col == 0 ? 0 : src[row * naxis1 + col - 1];
    }
}

// a block's code: every symbol's length and its code as the stream takes it, and the bits of the block's codes
struct BlockCode {
    int length[ro::DEFLATE_SYMS];
    uint32_t reversed[ro::DEFLATE_SYMS];
    uint32_t code_bits;
};

BlockCode block_code(const unsigned char *raw, int64_t len)
{
    uint32_t freq[ro::DEFLATE_SYMS] = {};
    for (int64_t i = 0; i < len; ++i) freq[raw[i]] += 1;
    freq[ro::DEFLATE_EOB] = 1;
    uint32_t key[ro::DEFLATE_SYMS];
    int n = 0;
    for (int s = 0; s < ro::DEFLATE_SYMS; ++s)
        if (freq[s]) key[n++] = ro::huff_key(freq[s], s);
    std::sort(key, key + n);
    ro::HuffWork work;
    int num[ro::DEFLATE_MAX_BITS + 1];
    ro::huff_counts(key, n, &work, num);
    // lengths in the order (frequency descending, symbol ascending)
    std::sort(key, key + n, [](uint32_t a, uint32_t b) { return (a >> 9) != (b >> 9) ? (a >> 9) > (b >> 9) : a < b; });
    BlockCode c{};
    for (int r = 0; r < n; ++r) c.length[key[r] & 0x1ffu] = ro::huff_length_at(num, r);
    uint32_t next[ro::DEFLATE_MAX_BITS + 1];
    ro::huff_first_codes(num, next);
    for (int s = 0; s < ro::DEFLATE_SYMS; ++s)
        if (c.length[s]) {
            c.reversed[s] = ro::huff_reverse(next[c.length[s]]++, c.length[s]);
            c.code_bits += freq[s] * (uint32_t)c.length[s];
        }
    return c;
}

// bits into bytes, the lowest bit of a byte first
struct BitWriter {
    unsigned char *out;
    uint64_t acc = 0;
    int held = 0;
    void put(uint32_t value, int bits)
    {
        acc |= (uint64_t)value << held;
        held += bits;
        for (; held >= 8; held -= 8, acc >>= 8) *out++ = (unsigned char)(acc & 0xffu);
    }
    void align()
    {
        if (held) put(0, 8 - held);
    }
};

// one block of `len` raw bytes at `out`, in the shorter form; the bytes written
int64_t write_block(const unsigned char *raw, int64_t len, bool last, unsigned char *out, bool measure_only)
{
    const BlockCode c = block_code(raw, len);
    const int64_t huffman = ro::deflate_huffman_bytes(c.code_bits, last);
    if (huffman >= 5 + len) {
        if (measure_only) return 5 + len;
        for (int j = 0; j < 5; ++j) out[j] = (unsigned char)ro::png_block_header_byte(j, last, (unsigned)len);
        std::memcpy(out + 5, raw, (size_t)len);
        return 5 + len;
    }
    if (measure_only) return huffman;
    BitWriter w{out};
    w.put(ro::deflate_prefix_word(0, last), 32);
    w.put(ro::deflate_prefix_word(1, last), 32);
    w.put(ro::deflate_prefix_word(2, last), ro::DEFLATE_PREFIX_BITS - 64);
    for (int s = 0; s < ro::DEFLATE_SYMS; ++s) w.put(ro::huff_reverse((uint32_t)c.length[s], 4), 4);
    w.put(0, 4);                                 // the one distance code: length 0
    for (int64_t i = 0; i < len; ++i) w.put(c.reversed[raw[i]], c.length[raw[i]]);
    w.put(c.reversed[ro::DEFLATE_EOB], c.length[ro::DEFLATE_EOB]);
    if (!last) w.put(0, 3);
    w.align();
    if (!last) w.put(0xffff0000u, 32);           // 00 00 FF FF
    return w.out - out;
}

// the blocks' bytes of one file, written at file + PNG_HEAD (file null: measured only)
int64_t write_blocks(const unsigned char *src, const ro::PngWant &w, unsigned char *file, uint32_t *adler)
{
    int64_t raw, blocks, idat;
    ro::png_shape(w.naxis1, w.naxis2, &raw, &blocks, &idat);
    std::vector<unsigned char> part((size_t)ro::PNG_STORED);
    int64_t stream = 0;
    uint32_t A = 1, B = 0;
    for (int64_t r0 = 0; r0 < raw; r0 += ro::PNG_STORED) {
        const int64_t len = std::min<int64_t>(raw - r0, ro::PNG_STORED);
        raw_bytes(src, w.naxis1, r0, len, part.data());
        stream += write_block(part.data(), len, r0 + len == raw, file ? file + ro::PNG_HEAD + stream : nullptr, !file);
        if (file)
            for (int64_t i = 0; i < len; ++i) {
                A = (A + part[(size_t)i]) % ro::ADLER_MOD;
                B = (B + A) % ro::ADLER_MOD;
            }
    }
    *adler = (B << 16) | A;
    return stream;
}

void write_file(const unsigned char *src, const ro::PngWant &w, unsigned char *file)
{
    uint32_t adler;
    const int64_t stream = write_blocks(src, w, file, &adler);
    const int64_t idat = ro::deflate_idat(stream), bytes = ro::deflate_file_bytes(stream);
    for (int i = 12; i < 29; ++i) file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)w.naxis1, (uint32_t)w.naxis2, 0, 0, false, 0);
    const uint32_t ihdr_crc = ~crc_bytes(0xffffffffu, file + 12, 17);
    for (int i = 0; i < ro::PNG_HEAD; ++i)
        file[i] = (unsigned char)ro::png_head_byte(i, (uint32_t)w.naxis1, (uint32_t)w.naxis2, ihdr_crc, (uint32_t)idat, false, 0);
    unsigned char *tail = file + ro::PNG_HEAD + stream;
    for (int i = 0; i < 4; ++i) tail[i] = (unsigned char)ro::png_tail_byte(i, adler, 0);
    const uint32_t crc = ~crc_bytes(0xffffffffu, file + 37, 4 + idat);
    for (int i = 4; i < ro::PNG_TAIL; ++i) tail[i] = (unsigned char)ro::png_tail_byte(i, adler, crc);
    std::memset(tail + ro::PNG_TAIL, 0, (size_t)(ro::png_room(bytes) - bytes));
}

}  // namespace

extern "C" int ro_stft_levels_png_deflate_resident(ro_stft_t *h, const ro_fits_unit_t *d_level_dir, int64_t dir_capacity,
                                                   const ro_unit_summary_t *d_level_summary, const void *d_levels,
                                                   int64_t levels_bytes, ro_fits_unit_t *d_png_dir, void *d_png, int64_t png_bytes,
                                                   ro_unit_summary_t *d_png_summary, void *stream)
{
    const char *who = "ro_stft_levels_png_deflate_resident";
    if (!h) return fail(RO_ERR_INVALID, "%s: null handle", who);
    int rc = png_check(who, "d_", true, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png, png_bytes,
                       d_png_summary);
    if (rc != RO_OK) return rc;
    ro::DeflateArgs a{};
    a.p.level_dir = d_level_dir;
    a.p.entries = &d_level_summary->entries;
    a.p.dir_capacity = dir_capacity;
    a.p.levels = static_cast<const unsigned char *>(d_levels);
    a.p.levels_bytes = levels_bytes;
    a.p.png_dir = d_png_dir;
    a.p.png = static_cast<char *>(d_png);
    a.p.png_bytes = png_bytes;
    a.p.summary = d_png_summary;
    HIP_TRY(hipSetDevice(h->device));
    int cus = 0;
    if ((rc = device_cus(h, &cus)) != RO_OK) return rc;
    if ((rc = grow_scratch(h->d_png_deflate_scratch, ro::deflate_scratch_bytes(dir_capacity, levels_bytes))) != RO_OK) return rc;
    ro::deflate_scratch_layout(a, h->d_png_deflate_scratch);
    HIP_TRY(ro::launch_levels_png_deflate(a, cus, (hipStream_t)stream));
    return RO_OK;
}

extern "C" int ro_levels_png_deflate_host(const ro_fits_unit_t *level_dir, int64_t dir_capacity,
                                          const ro_unit_summary_t *level_summary, const void *levels, int64_t levels_bytes,
                                          ro_fits_unit_t *png_dir, void *png, int64_t png_bytes, ro_unit_summary_t *png_summary)
{
    const char *who = "ro_levels_png_deflate_host";
    const int rc = png_check(who, "", false, level_dir, dir_capacity, level_summary, levels, levels_bytes, png_dir, png, png_bytes,
                             png_summary);
    if (rc != RO_OK) return rc;
    const int64_t n = entries_of(level_summary->entries, dir_capacity);
    const int64_t max_blocks = ro::deflate_max_blocks(dir_capacity, levels_bytes);
    ro_unit_summary_t sum{};
    sum.entries = n;
    int64_t first = 0;                           // rooms of every writable entry so far, fitting or not
    int64_t blocks = 0;                          // blocks of every entry rule 2 passes so far
    for (int64_t d = 0; d < n; ++d) {
        const ro_fits_unit_t &e = level_dir[d];
        ro::PngWant w = ro::png_want(e.offset, e.bytes, e.naxis2, e.naxis1, e.status, levels_bytes);
        if (w.status == RO_UNIT_WRITTEN) {
            blocks += w.blocks;
            if (blocks > max_blocks) w.status = RO_UNIT_INVALID;       // images that overlap each other beyond the bound
        }
        ro_fits_unit_t out{};
        out.status = w.status;
        if (w.status == RO_UNIT_SKIPPED) sum.skipped += 1;
        else if (w.status == RO_UNIT_INVALID) sum.invalid += 1;
        else {
            const unsigned char *src = static_cast<const unsigned char *>(levels) + w.source;
            uint32_t adler;
            const int64_t stream = write_blocks(src, w, nullptr, &adler);
            const int64_t bytes = ro::deflate_file_bytes(stream), room = ro::png_room(bytes);
            out.bytes = bytes;
            out.naxis2 = w.naxis2;
            out.naxis1 = w.naxis1;
            if (first + room <= png_bytes) {
                out.offset = first;
                write_file(src, w, static_cast<unsigned char *>(png) + first);
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
