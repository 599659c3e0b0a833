// ro_png_deflate.h -- the compressed preview files (ro_png_deflate.hip, ro_png_deflate.cpp): every level image of a level
// directory as a complete PNG whose deflate blocks are dynamic-Huffman blocks of literals only, or stored ones where those
// are not shorter (RFC 1951 3.2.2, 3.2.4, 3.2.7).  include/ro_stft.h states the file to the byte; this header has the
// arithmetic of a block -- the code lengths from the sorted frequencies, the limit to 15 bits, the block's header bits and
// its size -- shared by the kernels and the host's block coder (deflate_code, ro_png_deflate.cpp; the twin that walks the
// directory is in ro_png.cpp), and what the host side needs to launch.  The file around the blocks,
// the entry rule and the checksum constants are ro_png.h's.
#pragma once

#include "ro_png.h"

namespace ro {

constexpr int DEFLATE_SYMS = 257;                // the literals and end-of-block
constexpr int DEFLATE_EOB = 256;
constexpr int DEFLATE_MAX_BITS = 15;
constexpr int DEFLATE_PREFIX_BITS = 74;          // BFINAL, BTYPE, HLIT, HDIST, HCLEN and the 19 code-length-code lengths
constexpr int DEFLATE_HEAD_BITS = DEFLATE_PREFIX_BITS + 4 * (DEFLATE_SYMS + 1);      // 1106: ... and 258 four-bit lengths
constexpr uint32_t DEFLATE_UNUSED = 0xffffffffu; // the sort key of a symbol that does not occur: behind every used one

// the sort key of a used symbol: frequency (at most 65535) above the symbol, so that keys ascend by (frequency, symbol)
__host__ __device__ inline uint32_t huff_key(uint32_t freq, int symbol) { return (freq << 9) | (uint32_t)symbol; }

// what huff_counts works in: the internal nodes' weights, every node's parent and the internal nodes' depths
struct HuffWork {
    uint32_t weight[DEFLATE_SYMS - 1];
    uint16_t parent[2 * DEFLATE_SYMS - 1];
    uint16_t depth[DEFLATE_SYMS - 1];
};

// num[l], l = 1 ... 15: the leaves at depth l of the two-queue Huffman tree over key[0, n) (n >= 2 used symbols, ascending),
// after the limit rule.  Leaves wait in key order, internal nodes in the order they were made; a step joins the two smallest
// weights, a leaf before an internal node of equal weight.  Returns whether a leaf lay deeper than 15.
__host__ __device__ inline bool huff_counts(const uint32_t *key, int n, HuffWork *w, int *num)
{
    int leaf = 0, node = 0;
    for (int made = 0; made < n - 1; ++made) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool take_leaf = leaf < n && (node >= made || (key[leaf] >> 9) <= w->weight[node]);
            sum += take_leaf ? key[leaf] >> 9 : w->weight[node];
            w->parent[take_leaf ? leaf : n + node] = (uint16_t)(n + made);
            leaf += take_leaf ? 1 : 0;
            node += take_leaf ? 0 : 1;
        }
        w->weight[made] = sum;
    }
    // depths from the root (the node made last) down: a node's parent was made after it
    w->depth[n - 2] = 0;
    for (int i = n - 3; i >= 0; --i) w->depth[i] = (uint16_t)(w->depth[w->parent[n + i] - n] + 1);
    for (int l = 0; l <= DEFLATE_MAX_BITS; ++l) num[l] = 0;
    bool deeper = false;
    for (int i = 0; i < n; ++i) {
        const int d = w->depth[w->parent[i] - n] + 1;
        deeper = deeper || d > DEFLATE_MAX_BITS;
        num[d > DEFLATE_MAX_BITS ? DEFLATE_MAX_BITS : d] += 1;
    }
    int total = 0;
    for (int l = 1; l <= DEFLATE_MAX_BITS; ++l) total += num[l] << (DEFLATE_MAX_BITS - l);
    while (total != 1 << DEFLATE_MAX_BITS) {
        num[DEFLATE_MAX_BITS] -= 1;
        int l = DEFLATE_MAX_BITS - 1;
        while (num[l] == 0) --l;
        num[l] -= 1;
        num[l + 1] += 2;
        total -= 1;
    }
    return deeper;
}

// the length of the symbol at place `rank` of the order (frequency descending, symbol ascending): num[1] symbols of one
// bit first, then num[2] of two, ...
__host__ __device__ inline int huff_length_at(const int *num, int rank)
{
    int l = 1, below = num[1];
    while (l < DEFLATE_MAX_BITS && rank >= below) below += num[++l];
    return l;
}

// the first canonical code of every length (RFC 1951 3.2.2) from num[]
__host__ __device__ inline void huff_first_codes(const int *num, uint32_t *first)
{
    uint32_t code = 0;
    first[0] = 0;
    for (int l = 1; l <= DEFLATE_MAX_BITS; ++l) {
        code = (code + (l > 1 ? (uint32_t)num[l - 1] : 0u)) << 1;
        first[l] = code;
    }
}

// a code of `bits` bits as the stream takes it: its highest bit first, so bit-reversed in a word filled from bit 0 up
__host__ __device__ inline uint32_t huff_reverse(uint32_t code, int bits)
{
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) r |= ((code >> i) & 1u) << (bits - 1 - i);
    return r;
}

// bits [32 i, 32 i + 32) of a Huffman block's first 74: BFINAL, BTYPE = 2, HLIT = 0, HDIST = 0, HCLEN = 15, then the 19
// three-bit lengths in RFC order: 0 for 16, 17, 18 and 4 for 0 ... 15 (i < 3; bits from 74 on are zero)
__host__ __device__ inline uint32_t deflate_prefix_word(int i, bool final)
{
    uint32_t word = 0;
    for (int b = 32 * i; b < 32 * i + 32; ++b) {
        bool one = false;
        if (b == 0) one = final;
        else if (b == 2) one = true;                                   // BTYPE = 2: bits 1, 2 are 0, 1
        else if (b >= 13 && b < 17) one = true;                        // HCLEN = 15
        else if (b >= 26 && b < DEFLATE_PREFIX_BITS) one = (b - 26) % 3 == 2;      // the value 4, lowest bit first
        word |= (one ? 1u : 0u) << (b - 32 * i);
    }
    return word;
}

// the bytes of a block's Huffman form with its ending, from the bits of its codes (end-of-block's included): a block that
// is not the last has 000, zero bits up to the byte boundary and 00 00 FF FF behind it
__host__ __device__ inline uint32_t deflate_huffman_bytes(uint32_t code_bits, bool last)
{
    return (DEFLATE_HEAD_BITS + code_bits + (last ? 0u : 3u) + 7u) / 8u + (last ? 0u : 4u);
}

// the file around `stream` bytes of blocks: the IDAT length and the file's bytes
__host__ __device__ inline int64_t deflate_idat(int64_t stream) { return 2 + stream + 4; }
__host__ __device__ inline int64_t deflate_file_bytes(int64_t stream) { return 8 + 25 + 12 + deflate_idat(stream) + 12; }

// The blocks of all valid entries that the calls measure: a level image of p pixels has at most 2 p raw bytes, so images
// that lie side by side in levels_bytes have no more.  Entries whose blocks pass it are RO_UNIT_INVALID (include/ro_stft.h)
inline int64_t deflate_max_blocks(int64_t dir_capacity, int64_t levels_bytes) { return levels_bytes / PNG_STORED * 2 + 1 + dir_capacity; }
// (2 x / 65535 rounded down is at most that, and nothing overflows)

// ---- the device call's scratch ------------------------------------------------------------------------------------------------
// what the measure leaves of a block, and the sum adds: the block's bytes in the stream, its form, the stream bytes of its
// file in front of it
struct DeflateBlock {
    uint32_t bytes, huffman, before, code_bits;
};
// a block's table: for every symbol its length above its bit-reversed code, 0 for an unused one
constexpr int DEFLATE_TABLE_WORDS = 260;

struct DeflateArgs {
    PngArgs        p;                            // the sources, the outputs; head, first_block and parts of the scratch
    int64_t       *stream;                       // scratch: [dir_capacity] the blocks' bytes of every measured entry's file
    DeflateBlock  *blocks;                       // scratch: [p.max_blocks]
    uint32_t      *tables;                       // scratch: [p.max_blocks][DEFLATE_TABLE_WORDS]
};

size_t deflate_scratch_bytes(int64_t dir_capacity, int64_t levels_bytes);
void deflate_scratch_layout(DeflateArgs &a, void *scratch);

// want, measure, sum, place, emit, finish on `s`: six launches; cus: the device's compute units
hipError_t launch_levels_png_deflate(const DeflateArgs &a, int cus, hipStream_t s);

}  // namespace ro
