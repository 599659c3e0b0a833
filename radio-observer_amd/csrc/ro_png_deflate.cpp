// ro_png_deflate.cpp -- the compressed preview files (include/ro_stft.h; kernels: ro_png_deflate.hip): every level image of a
// level directory as a complete PNG whose deflate blocks are Huffman coded where that is shorter: argument checks, the
// handle's scratch, the launches; and a deflate block on the host, for the file writer of ro_png.cpp: its code by the rules of
// ro_png_deflate.h, and its bytes in either form through a bit writer.  Nothing in the resident call reads device memory.
#include "ro_host.h"

using namespace ro::host;

namespace {

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

}  // namespace

DeflateCode ro::host::deflate_code(const unsigned char *raw, int64_t len, bool last)
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
    DeflateCode c{};
    for (int r = 0; r < n; ++r) c.length[key[r] & 0x1ffu] = (uint8_t)ro::huff_length_at(num, r);
    uint32_t next[ro::DEFLATE_MAX_BITS + 1];
    ro::huff_first_codes(num, next);
    uint32_t code_bits = 0;
    for (int s = 0; s < ro::DEFLATE_SYMS; ++s)
        if (c.length[s]) {
            c.reversed[s] = (uint16_t)ro::huff_reverse(next[c.length[s]]++, c.length[s]);
            code_bits += freq[s] * (uint32_t)c.length[s];
        }
    const int64_t huffman = ro::deflate_huffman_bytes(code_bits, last);
    c.huffman = huffman < 5 + len;
    c.bytes = c.huffman ? huffman : 5 + len;
    return c;
}

int64_t ro::host::deflate_write_block(const unsigned char *raw, int64_t len, bool last, const DeflateCode *code, unsigned char *out)
{
    if (!code || !code->huffman) {
        for (int j = 0; j < 5; ++j) out[j] = (unsigned char)ro::png_block_header_byte(j, last, (unsigned)len);
        std::memcpy(out + 5, raw, (size_t)len);
        return 5 + len;
    }
    BitWriter w{out};
    w.put(ro::deflate_prefix_word(0, last), 32);
    w.put(ro::deflate_prefix_word(1, last), 32);
    w.put(ro::deflate_prefix_word(2, last), ro::DEFLATE_PREFIX_BITS - 64);
    for (int s = 0; s < ro::DEFLATE_SYMS; ++s) w.put(ro::huff_reverse(code->length[s], 4), 4);
    w.put(0, 4);                                 // the one distance code: length 0
    for (int64_t i = 0; i < len; ++i) w.put(code->reversed[raw[i]], code->length[raw[i]]);
    w.put(code->reversed[ro::DEFLATE_EOB], code->length[ro::DEFLATE_EOB]);
    if (!last) w.put(0, 3);
    w.align();
    if (!last) w.put(0xffff0000u, 32);           // 00 00 FF FF
    return w.out - out;
}

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
    png_fill_args(a.p, d_level_dir, dir_capacity, d_level_summary, d_levels, levels_bytes, d_png_dir, d_png, png_bytes, d_png_summary);
    int cus = 0;
    if ((rc = scratch_for(h, h->d_png_deflate_scratch, ro::deflate_scratch_bytes(dir_capacity, levels_bytes), &cus)) != RO_OK) return rc;
    ro::deflate_scratch_layout(a, h->d_png_deflate_scratch);
    HIP_TRY(ro::launch_levels_png_deflate(a, cus, (hipStream_t)stream));
    return RO_OK;
}
