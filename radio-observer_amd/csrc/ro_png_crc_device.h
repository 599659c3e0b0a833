// ro_png_crc_device.h -- device helpers of the preview files' kernels (ro_png.hip, ro_png_deflate.hip): the raw bytes of an
// image of scanlines, the CRC-32 steps over the tables of ro_png.h, and the wave's sums.  Device code only.
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

}  // namespace ro
