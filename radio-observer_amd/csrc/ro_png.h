// ro_png.h -- the preview files on the device (ro_png.hip): every level image of a level directory as a complete PNG whose
// zlib stream uses stored deflate blocks (RFC 1950, RFC 1951 3.2.4, PNG 1.2 chapters 3, 5 and 11).  include/ro_stft.h
// states the file to the byte and the entry rules; this header has the arithmetic of that file, the entry rule and the
// checksum constants, shared by the kernels and the host twin (ro_png.cpp), and what the host side needs to launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"

// entries of one tile of png_plan_kernel: one per lane of its one workgroup, four waves
#define RO_PNG_TILE 256

namespace ro {

constexpr int64_t PNG_MAX_ENTRIES = (int64_t)1 << 24;
constexpr int64_t PNG_STORED = 65535;            // raw bytes of a stored deflate block but the last
constexpr int64_t PNG_PITCH = PNG_STORED + 5;    // file bytes from one block's header to the next one's
constexpr int64_t PNG_HEAD = 43;                 // file byte of block 0's header: signature 8, IHDR 25, IDAT length and type 8, zlib 2
constexpr int64_t PNG_DATA = PNG_HEAD + 5;       // ... of its first raw byte
constexpr int64_t PNG_TAIL = 20;                 // Adler-32, the IDAT CRC, IEND
constexpr int64_t PNG_IDAT_MAX = 0x7fffffff;     // a chunk's length field

// raw bytes (a filter byte and naxis1 levels per scanline), stored blocks and the IDAT length of an image; false: not a PNG
__host__ __device__ inline bool png_shape(int32_t naxis1, int64_t naxis2, int64_t *raw, int64_t *blocks, int64_t *idat)
{
    if (naxis1 < 1 || naxis2 < 1 || naxis2 > PNG_IDAT_MAX) return false;
    const int64_t r = naxis2 * ((int64_t)naxis1 + 1);                  // below 2^62
    if (r > PNG_IDAT_MAX) return false;
    const int64_t n = (r + PNG_STORED - 1) / PNG_STORED;
    const int64_t len = 6 + 5 * n + r;
    if (len > PNG_IDAT_MAX) return false;
    *raw = r;
    *blocks = n;
    *idat = len;
    return true;
}

// ro_png_bytes: 63 + 5 blocks + raw, or -1
__host__ __device__ inline int64_t png_file_bytes(int32_t naxis1, int64_t naxis2)
{
    int64_t raw, blocks, idat;
    return png_shape(naxis1, naxis2, &raw, &blocks, &idat) ? 8 + 25 + 12 + idat + 12 : -1;
}

// What one level entry asks for, before the room is looked at: RO_UNIT_SKIPPED, RO_UNIT_INVALID, or RO_UNIT_WRITTEN for a
// writable one with its shape, where its levels start, its file's bytes and its stored blocks (rules 1 - 3)
struct PngWant {
    int32_t status;
    int32_t naxis1;
    int64_t naxis2;
    int64_t source;                // byte of the levels that is pixel 0
    int64_t bytes;                 // the file's
    int64_t blocks;
};

__host__ __device__ inline PngWant png_want(int64_t offset, int64_t bytes, int64_t naxis2, int32_t naxis1, int32_t status,
                                            int64_t levels_bytes)
{
    PngWant w = {RO_UNIT_SKIPPED, 0, 0, 0, 0, 0};
    if (status != RO_UNIT_WRITTEN) return w;
    w.status = RO_UNIT_INVALID;
    int64_t raw, blocks, idat;
    // (the shape first: what it passes has naxis1 naxis2 below 2^31)
    if (!png_shape(naxis1, naxis2, &raw, &blocks, &idat) || bytes != (int64_t)naxis1 * naxis2 || offset < 0 ||
        offset % RO_LEVEL_BLOCK != 0 || offset > levels_bytes || bytes > levels_bytes - offset)
        return w;
    w.status = RO_UNIT_WRITTEN;
    w.naxis1 = naxis1;
    w.naxis2 = naxis2;
    w.source = offset;
    w.bytes = png_file_bytes(naxis1, naxis2);
    w.blocks = blocks;
    return w;
}

// what a file occupies: its bytes rounded up to RO_PNG_ALIGN
__host__ __device__ inline int64_t png_room(int64_t bytes) { return (bytes + RO_PNG_ALIGN - 1) / RO_PNG_ALIGN * RO_PNG_ALIGN; }

// byte i of the 5-byte header of a stored block of `len` raw bytes
__host__ __device__ inline unsigned png_block_header_byte(int i, bool final, unsigned len)
{
    const unsigned nlen = ~len & 0xffffu;
    return i == 0 ? (final ? 1u : 0u) : i == 1 ? (len & 0xffu) : i == 2 ? (len >> 8) : i == 3 ? (nlen & 0xffu) : (nlen >> 8);
}

// byte i < PNG_DATA of a file: the signature, IHDR (8 bit, grey, no interlace) with its CRC, the IDAT length and type, the
// zlib header 78 01 and block 0's header
__host__ __device__ inline unsigned png_head_byte(int i, uint32_t naxis1, uint32_t naxis2, uint32_t ihdr_crc, uint32_t idat,
                                                  bool final0, unsigned len0)
{
    const unsigned char fixed[16] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
    const unsigned char type[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
    auto be = [](uint32_t v, int k) { return (v >> (24 - 8 * k)) & 0xffu; };
    if (i < 16) return fixed[i];
    if (i < 20) return be(naxis1, i - 16);
    if (i < 24) return be(naxis2, i - 20);
    if (i < 29) return i == 24 ? 8u : 0u;
    if (i < 33) return be(ihdr_crc, i - 29);
    if (i < 37) return be(idat, i - 33);
    if (i < 43) return type[i - 37];
    return png_block_header_byte(i - 43, final0, len0);
}

// byte i < PNG_TAIL behind the last raw byte: the Adler-32, the IDAT CRC, and the IEND chunk
__host__ __device__ inline unsigned png_tail_byte(int i, uint32_t adler, uint32_t crc)
{
    const unsigned char iend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xae, 0x42, 0x60, 0x82};
    if (i < 4) return (adler >> (24 - 8 * i)) & 0xffu;
    if (i < 8) return (crc >> (24 - 8 * (i - 4))) & 0xffu;
    return iend[i - 8];
}

// ---- CRC-32 (PNG 1.2 annex 15, zlib's crc32): the reflected polynomial, a word's bit 31 the coefficient of x^0.  A
// register state after a message is linear in (state before, message): from state 0 it is the message's remainder, and n
// zero bytes multiply a state by x^(8 n) mod P.  So the remainder of A || B is rem(A) x^(8 |B|) + rem(B), and the CRC is
// rem(M) + 0xffffffff x^(8 |M|) + 0xffffffff.
constexpr uint32_t CRC_POLY = 0xedb88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;        // x^0
constexpr uint32_t ADLER_MOD = 65521u;

// a(x) b(x) mod P
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= (a & (CRC_ONE >> i)) ? b : 0u;
        b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u);
    }
    return p;
}

// The tables.  byte[k][v]: the state that byte v of a little-endian word leaves when it is byte k of four absorbed at once
// (k = 3: the plain byte table); gap[k][v]: the same with 1020 zero bytes behind the word, for a lane that takes every
// 256th word; lane[t] = x^(32 t), what brings lane t's state to the end of the last word; x2n[j] = x^(2^j)
struct PngTables {
    uint32_t byte[4][256], gap[4][256], lane[256], x2n[32];
};
constexpr int PNG_LANES = 256;                   // lanes of a workgroup of png_blocks_kernel; the gap is 4 (PNG_LANES - 1) bytes

// x^(8 n) from the squares: x^(2^32) = x (zlib's x2nmodp)
__host__ __device__ constexpr uint32_t crc_xpow8(const uint32_t (&x2n)[32], uint64_t n)
{
    uint32_t p = CRC_ONE;
    for (int j = 0; n; n >>= 1, ++j)
        if (n & 1u) p = crc_mul(p, x2n[(j + 3) & 31]);
    return p;
}

constexpr PngTables make_png_tables()
{
    PngTables t = {};
    t.x2n[0] = CRC_ONE >> 1;
    for (int j = 1; j < 32; ++j) t.x2n[j] = crc_mul(t.x2n[j - 1], t.x2n[j - 1]);
    const uint32_t gap = crc_xpow8(t.x2n, 4 * (PNG_LANES - 1)), word = crc_xpow8(t.x2n, 4);
    // every table is linear in v: the eight single bits first, the rest by the lowest bit
    for (int bit = 0; bit < 8; ++bit) {
        uint32_t c = 1u << bit;
        for (int i = 0; i < 8; ++i) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u);
        for (int k = 3; k >= 0; --k) {
            t.byte[k][1 << bit] = c;
            t.gap[k][1 << bit] = crc_mul(c, gap);
            uint32_t z = c;                      // one more zero byte
            for (int i = 0; i < 8; ++i) z = (z >> 1) ^ ((z & 1u) ? CRC_POLY : 0u);
            c = z;
        }
    }
    for (int k = 0; k < 4; ++k)
        for (int v = 1; v < 256; ++v) {
            const int low = v & -v;
            t.byte[k][v] = t.byte[k][v ^ low] ^ t.byte[k][low];
            t.gap[k][v] = t.gap[k][v ^ low] ^ t.gap[k][low];
        }
    t.lane[0] = CRC_ONE;
    for (int i = 1; i < PNG_LANES; ++i) t.lane[i] = crc_mul(t.lane[i - 1], word);
    return t;
}

// png_plan_kernel -> png_blocks_kernel -> png_finish_kernel: first_block[d] is the stored block of all files where entry
// d's file starts, or would start if it had one: the exclusive prefix of the writable entries' blocks, never descending
struct PngPlanHead {
    int64_t entries;               // entries of the directory and of first_block
    int64_t blocks;                // stored blocks of all WRITTEN files
};

// blocks -> finish: what a stored block, with its header (block 0: with the chunk type and the zlib header too), adds to
// the file's checksums whatever the order they are added in: its remainder times x^(8 x the IDAT bytes behind it), its
// bytes' sum, and the sum of its bytes times the raw bytes from each to the image's end, the last two mod 65521
struct PngPart {
    uint32_t crc, a, b, reserved;
};

struct PngArgs {
    const ro_fits_unit_t *level_dir;             // null with dir_capacity 0
    const int64_t        *entries;               // the level summary's first word
    int64_t               dir_capacity;
    const unsigned char  *levels;
    int64_t               levels_bytes;
    ro_fits_unit_t       *png_dir;
    char                 *png;
    int64_t               png_bytes;
    ro_unit_summary_t    *summary;
    PngPlanHead          *head;                  // scratch
    int64_t              *first_block;           // scratch: [dir_capacity]
    PngPart              *parts;                 // scratch: [max_blocks]
    int64_t               max_blocks;
};

// The stored blocks of files that lie side by side in png_bytes: a file of n blocks has more than 65535 (n - 1) bytes
inline int64_t png_max_blocks(int64_t dir_capacity, int64_t png_bytes) { return png_bytes / PNG_STORED + dir_capacity; }

// bytes of scratch a call needs (16-byte aligned device memory), and its layout into head / parts / first_block
size_t png_scratch_bytes(int64_t dir_capacity, int64_t png_bytes);
void png_scratch_layout(PngArgs &a, void *scratch);

// the plan, the blocks and the finish on `s`: three launches; cus: the device's compute units
hipError_t launch_levels_png(const PngArgs &a, int cus, hipStream_t s);

// what the launchers of both kinds of file (ro_png.hip, ro_png_deflate.hip) ask of the arguments they share, but max_blocks
inline bool png_args_valid(const PngArgs &a)
{
    return a.dir_capacity >= 0 && a.dir_capacity <= PNG_MAX_ENTRIES && (a.dir_capacity == 0 || a.level_dir) && a.entries &&
           a.levels_bytes >= 0 && (a.levels_bytes == 0 || a.levels) && a.png_dir && a.png_bytes >= 0 && (a.png_bytes == 0 || a.png) &&
           ((uintptr_t)a.png & (RO_PNG_ALIGN - 1)) == 0 && a.summary && a.head && a.first_block && a.parts;
}
// ... and their grids: of the `most` workgroups of a copy (copy_grid, ro_pack_plan.h) no more than there are items for them,
// `per_group` to a workgroup
inline unsigned png_grid_for(unsigned most, int64_t items, int per_group)
{
    const int64_t need = (items + per_group - 1) / per_group;
    return (unsigned)(need < 1 ? 1 : need < (int64_t)most ? need : (int64_t)most);
}

}  // namespace ro
