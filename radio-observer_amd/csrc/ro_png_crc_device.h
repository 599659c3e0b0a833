// ro_png_crc_device.h -- device helpers of the preview files' kernels (ro_png.hip, ro_png_deflate.hip): the raw bytes of an
// image of scanlines, the CRC-32 steps over the tables of ro_png.h, the wave's sums, and what both files' kernels do the
// same way once per entry or per block: the read of a level entry, the store of the summary, the fold of the waves' sums and
// a block's part of the file's checksums.  (The two finish kernels keep their bodies: as a shared function the same lines
// cost png_finish_kernel one more SGPR, profiles/png_refactor.txt.)  Device code only.
#pragma once

#include "ro_pack_plan.h"
#include "ro_png.h"

namespace ro {

// raw byte i of an image of scanlines of w levels: the filter byte in front of a scanline, else a level
__device__ __forceinline__ unsigned raw_byte(const unsigned char *__restrict__ src, unsigned w, unsigned i)
{
    const unsigned row = i / (w + 1), col = i - row * (w + 1);
    const unsigned v = src[(int64_t)row * w + (col ? col - 1 : 0)];
    return col ? v : 0u;
}

// raw bytes i ... i + 3, the first one lowest: one division, then the scanline's end is stepped over (w may be 1).  No
// load is guarded: a filter byte reads its scanline's first level and drops it
__device__ __forceinline__ unsigned raw_word(const unsigned char *__restrict__ src, unsigned w, unsigned i)
{
    const unsigned row = i / (w + 1);
    unsigned col = i - row * (w + 1);
    const unsigned char *p = src + (int64_t)row * w;
    unsigned word = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned v = p[col ? col - 1 : 0];
        word |= (col ? v : 0u) << (8 * j);
        const bool wrap = col == w;
        col = wrap ? 0u : col + 1;
        p += wrap ? w : 0u;
    }
    return word;
}

__device__ __forceinline__ uint32_t crc_byte(const PngTables &tab, uint32_t c, unsigned v)
{
    return tab.byte[3][(c ^ v) & 0xffu] ^ (c >> 8);
}
// four bytes at once, and with the zero bytes up to the lane's next word behind them
__device__ __forceinline__ uint32_t crc_word(const uint32_t (&t)[4][256], uint32_t c)
{
    return t[0][c & 0xffu] ^ t[1][(c >> 8) & 0xffu] ^ t[2][(c >> 16) & 0xffu] ^ t[3][c >> 24];
}
// without a table, for the few bytes of png_finish_kernel
__device__ __forceinline__ uint32_t crc_byte_plain(uint32_t c, unsigned v)
{
    c ^= v;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
    return c;
}

// x^(8 e) in every lane of a half wave, e the same in all of its 32 lanes: lane j holds the square of e's bit j, and five
// exchanges multiply them (the two halves may ask for different e)
__device__ __forceinline__ uint32_t wave_xpow8(const uint32_t (&x2n)[32], uint32_t e, int lane)
{
    const int j = lane & 31;
    uint32_t p = ((e >> j) & 1u) ? x2n[(j + 3) & 31] : CRC_ONE;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) p = crc_mul(p, (uint32_t)__shfl_xor((int)p, off));
    return p;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t x)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x ^= (uint32_t)__shfl_xor((int)x, off);
    return x;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) x += (uint32_t)__shfl_xor((int)x, off);
    return x;
}

// ---- what the two files' kernels do once per entry, per block or per file, outside every loop over bytes

// what level entry d asks for: the entry read as its four words (no guarded load of a struct)
__device__ __forceinline__ PngWant png_want_entry(const ro_fits_unit_t *level_dir, int64_t d, int64_t levels_bytes)
{
    const int64_t *e = reinterpret_cast<const int64_t *>(level_dir + d);
    const int64_t e3 = e[3];
    return png_want(e[0], e[1], e[2], (int32_t)(uint32_t)e3, (int32_t)(uint32_t)((uint64_t)e3 >> 32), levels_bytes);
}

// the files' summary, stored by the one thread that calls this
__device__ __forceinline__ void png_store_summary(ro_unit_summary_t *summary, int64_t entries, int64_t written, int64_t skipped,
                                                  int64_t no_room, int64_t invalid, int64_t used, int64_t needed)
{
    ro_unit_summary_t sum;
    sum.entries = entries;
    sum.written = written;
    sum.skipped = skipped;
    sum.no_room = no_room;
    sum.invalid = invalid;
    sum.units_bytes = used;
    sum.needed_bytes = needed;
    sum.reserved = 0;
    *summary = sum;
}

// the waves' sums of one block, as each wave's lane 0 left them in LDS, folded: the CRC state and the two Adler sums
template <int N>
__device__ __forceinline__ void png_fold(const uint32_t (&red)[PLAN_WAVES][N], uint32_t &c, uint32_t &A, uint32_t &B)
{
    c = A = B = 0u;
#pragma unroll
    for (int v = 0; v < PLAN_WAVES; ++v) {
        c ^= red[v][0];
        A += red[v][1];
        B += red[v][2];
    }
}

// The part of one block (PngPart): c the state over the block's bytes, pre the state over what stands in front of them in
// the chunk, power and power_block x to 8 times the IDAT bytes behind the block and behind its first byte; A and B the
// block's Adler sums, `raw_behind` the image's raw bytes behind the block
__device__ __forceinline__ PngPart png_part(uint32_t c, uint32_t A, uint32_t B, uint32_t pre, uint32_t power, uint32_t power_block,
                                            unsigned raw_behind)
{
    PngPart part;
    part.crc = crc_mul(pre, power_block) ^ crc_mul(c, power);
    part.a = A % ADLER_MOD;
    part.b = (uint32_t)((B % ADLER_MOD + (uint64_t)(raw_behind % ADLER_MOD) * part.a) % ADLER_MOD);
    part.reserved = 0u;
    return part;
}

}  // namespace ro
