// ro_png_deflate.hip -- the compressed preview files on the device: every level image of a level directory as a complete PNG
// whose deflate blocks of 65535 raw bytes are dynamic-Huffman blocks of literals only, or stored ones where those are not
// shorter.  include/ro_stft.h states the file to the byte and the entry rules; ro_png_deflate.h has a block's arithmetic (the
// two-queue construction, the limit to 15 bits, the header bits), which the host twin runs too; ro_png.h the file around the
// blocks and the checksum constants.  Nothing is remembered from call to call and the levels and their directory are only read.
//
// Plain launches; no workgroup waits for another one of its launch, no global atomics, no floating point, and every result
// is integer arithmetic that does not depend on the order of its terms (LDS adds and ORs), so the same input gives the same
// bytes.  Sizes depend on the data, so the plan comes after a measurement: want, measure, place, emit, finish, with the place
// in two launches, because a file of many blocks is summed by a wave and not by a lane of the one workgroup that scans the rooms:
//   deflate_want_kernel     the entry rules over the level directory and the exclusive prefix of the valid entries' blocks
//                           (first_block), over every valid entry, fitting or not: the sizing call measures them too
//   deflate_measure_kernel  a workgroup takes a block: the histogram of its raw bytes in LDS, one per wave, folded; the used
//                           (frequency, symbol) keys ranked against each other, ascending for the construction and descending
//                           for the lengths; one lane runs huff_counts (the joins, the depths, the limit); every lane gives
//                           its symbol its length and its canonical code.  It leaves the block's table (length and
//                           bit-reversed code per symbol), its form and its bytes in scratch
//   deflate_sum_kernel      a wave takes a file: the scan of its blocks' bytes -- where each block starts in the file's stream --
//                           and their sum
//   deflate_place_kernel    the plan of ro_pack_plan.h over the files' ACTUAL rooms: the directory and the summary
//   deflate_emit_kernel     a workgroup takes a block of a written file and assembles its bytes in LDS, at the block's own
//                           position within a word of the file (a block starts at any byte).  Huffman form: the header bits;
//                           each lane takes a contiguous run of raw bytes, a workgroup scan of the runs' bits gives it its bit
//                           offset, and it ORs its codes into LDS a word at a time.  Stored form: the header and the raw words.
//                           Then lanes on every 256th word store them (the partial words at both ends byte by byte: they
//                           are shared with the neighbours) and run the CRC-32 of ro_png.hip's scheme over them; the Adler
//                           parts come from the raw bytes.  Block 0's workgroup writes the file's first 43 bytes too
//   deflate_finish_kernel   a wave takes a file: adds its blocks' parts, writes the Adler-32, the IDAT CRC, IEND and the zeros
//                           up to the next multiple of 16
// Every level byte is read three times (histogram; the runs' bits; the codes), the last two from cache; one staged block of
// 64 KiB and the tables make 76 KiB of LDS, two workgroups per CU.
#include "ro_pack_plan.h"
#include "ro_png_deflate.h"
#include "ro_png_crc_device.h"

namespace ro {

namespace {

constexpr int T = RO_PNG_TILE;
static_assert(T == PLAN_TILE && T == PNG_LANES && T == 256, "one entry or symbol per lane, four waves");
static_assert(sizeof(DeflateBlock) == 16 && sizeof(PngPart) == 16 && DEFLATE_TABLE_WORDS >= DEFLATE_SYMS, "the scratch's layout");

// a staged block: up to 3 bytes of the file's word in front of it, its bytes, and a word to spare
constexpr int STAGE_WORDS = (3 + (int)PNG_PITCH + 3) / 4 + 1;

__device__ const PngTables TABLES = make_png_tables();

// The entry rules and the blocks' prefix.  An entry is MEASURED when rule 2 passes it and the blocks up to and including its
// own are at most max_blocks.
__global__ __launch_bounds__(T) void deflate_want_kernel(DeflateArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wsum[1][PLAN_WAVES], wend[1][PLAN_WAVES];
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];
    int64_t n = *a.p.entries;
    n = n < 0 ? 0 : (n > a.p.dir_capacity ? a.p.dir_capacity : n);
    int64_t block_base = 0, measured = 0;
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int64_t c = t0 + threadIdx.x;
        const PngWant w = png_want_entry(a.p.level_dir, c < n ? c : n - 1, a.p.levels_bytes);
        const bool live = c < n;
        const bool valid = live && w.status == RO_UNIT_WRITTEN;
        const int64_t take[1] = {valid ? w.blocks : 0};
        const TileScan<1> scan = tile_scan(take, wsum, lane, wave);
        const int64_t first_b = block_base + scan.before[0];
        const bool is[PLAN_CLASSES] = {valid && first_b + take[0] <= a.p.max_blocks, false, false, false};
        const int64_t end[1] = {first_b + take[0]};
        const TileCount<1> count = tile_count(is, end, wcnt, wend, lane, wave);
        measured = count.end[0] > measured ? count.end[0] : measured;
        if (live) a.p.first_block[c] = first_b;
        block_base += scan.total[0];
    }
    if (threadIdx.x == 0) {
        PngPlanHead head;
        head.entries = n;
        head.blocks = measured < a.p.max_blocks ? measured : a.p.max_blocks;
        *a.p.head = head;
    }
}

// a measured entry as the want left it, checked once more against the buffers before anything of it is touched
struct DeflateSource {
    const unsigned char *src;      // level of pixel 0
    unsigned naxis1, raw, blocks;
    int64_t naxis2;
    int64_t first_block;
};

__device__ __forceinline__ bool deflate_source(const DeflateArgs &a, int64_t d, DeflateSource &f)
{
    const int64_t first = a.p.first_block[d];
    const PngWant w = png_want_entry(a.p.level_dir, d, a.p.levels_bytes);
    int64_t raw, blocks, idat;
    if (w.status != RO_UNIT_WRITTEN || !png_shape(w.naxis1, w.naxis2, &raw, &blocks, &idat) || first < 0 ||
        first > a.p.max_blocks || blocks > a.p.max_blocks - first)
        return false;
    f.src = a.p.levels + w.source;
    f.naxis1 = (unsigned)w.naxis1;
    f.naxis2 = w.naxis2;
    f.raw = (unsigned)raw;
    f.blocks = (unsigned)blocks;
    f.first_block = first;
    return true;
}

// the block of work item b: its entry's source, its first raw byte, its raw bytes; false: no work
struct DeflateItem {
    int64_t d;
    unsigned k, r0, len;
    bool last;
};
__device__ __forceinline__ bool deflate_item(const DeflateArgs &a, int64_t entries, int64_t b, DeflateSource &f, DeflateItem &it)
{
    it.d = plan_entry(a.p.first_block, entries, b);
    if (it.d < 0 || !deflate_source(a, it.d, f)) return false;
    const int64_t k64 = b - f.first_block;
    if (k64 >= f.blocks) return false;
    it.k = (unsigned)k64;
    it.r0 = it.k * (unsigned)PNG_STORED;
    it.len = f.raw - it.r0 < PNG_STORED ? f.raw - it.r0 : (unsigned)PNG_STORED;
    it.last = it.k + 1 == f.blocks;
    return true;
}

// raw bytes i ... i + 3 of a block of len, the first one lowest, zeros behind the block's end; n: how many are the block's
__device__ __forceinline__ unsigned block_word(const DeflateSource &f, unsigned r0, unsigned len, unsigned i, unsigned &n)
{
    if (i + 4u <= len) {
        n = 4u;
        return raw_word(f.src, f.naxis1, r0 + i);
    }
    unsigned word = 0u;
    n = i < len ? len - i : 0u;
    for (unsigned q = 0; q < n; ++q) word |= raw_byte(f.src, f.naxis1, r0 + i + q) << (8 * q);
    return word;
}

// where symbol s stands among the used symbols: by (frequency, symbol) ascending, and by (frequency descending, symbol
// ascending); every lane reads the same word of freq[] at a time
__device__ __forceinline__ void huff_ranks(const uint32_t *freq, int s, int &ascending, int &descending, int &used)
{
    const uint32_t f = freq[s];
    int asc = 0, desc = 0, n = 0;
    for (int o = 0; o < DEFLATE_SYMS; ++o) {
        const uint32_t g = freq[o];
        const bool in = g != 0u, tie = g == f && o < s;
        asc += (in && (g < f || tie)) ? 1 : 0;
        desc += (in && (g > f || tie)) ? 1 : 0;
        n += in ? 1 : 0;
    }
    ascending = asc;
    descending = desc;
    used = n;
}

// the table entry of symbol s: its length above its canonical code, bit-reversed; 0 for an unused symbol
__device__ __forceinline__ uint32_t huff_entry(const uint32_t *length, const uint32_t *first_code, int s)
{
    const uint32_t l = length[s];
    uint32_t same = 0;
    for (int o = 0; o < DEFLATE_SYMS; ++o) same += (o < s && length[o] == l) ? 1u : 0u;
    return l ? (l << 16) | (__brev(first_code[l] + same) >> (32u - l)) : 0u;
}

// The measure: a work item is a block of a measured entry, a workgroup takes it.
__global__ __launch_bounds__(T) void deflate_measure_kernel(DeflateArgs a)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t total = a.p.head->blocks, entries = a.p.head->entries;
    __shared__ uint32_t hist[PLAN_WAVES][256];
    __shared__ uint32_t freq[DEFLATE_SYMS], key[DEFLATE_SYMS], length[DEFLATE_SYMS], first_code[DEFLATE_MAX_BITS + 1];
    __shared__ HuffWork work;
    __shared__ int num[DEFLATE_MAX_BITS + 1];
    __shared__ uint32_t wbits[PLAN_WAVES];
    for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
        DeflateSource f;
        DeflateItem it;
        if (!deflate_item(a, entries, b, f, it)) continue;
#pragma unroll
        for (int v = 0; v < PLAN_WAVES; ++v) hist[v][t] = 0u;
        wg_sync();
        const unsigned words = (it.len + 3u) >> 2;
        for (unsigned j = (unsigned)t; j < words; j += (unsigned)T) {
            unsigned n;
            const unsigned v = block_word(f, it.r0, it.len, 4u * j, n);
#pragma unroll
            for (unsigned q = 0; q < 4u; ++q)
                if (q < n) atomicAdd(&hist[wave][(v >> (8u * q)) & 0xffu], 1u);
        }
        wg_sync();
        freq[t] = hist[0][t] + hist[1][t] + hist[2][t] + hist[3][t];
        if (t == 0) freq[DEFLATE_EOB] = 1u;
        wg_sync();
        int asc, desc, used, desc_eob = 0;
        huff_ranks(freq, t, asc, desc, used);
        if (freq[t]) key[asc] = huff_key(freq[t], t);
        if (t == 0) {
            int asc_eob, used_eob;
            huff_ranks(freq, DEFLATE_EOB, asc_eob, desc_eob, used_eob);
            key[asc_eob] = huff_key(1u, DEFLATE_EOB);
        }
        wg_sync();
        if (t == 0) {
            huff_counts(key, used, &work, num);
            huff_first_codes(num, first_code);
        }
        wg_sync();
        length[t] = freq[t] ? (uint32_t)huff_length_at(num, desc) : 0u;
        if (t == 0) length[DEFLATE_EOB] = (uint32_t)huff_length_at(num, desc_eob);
        wg_sync();
        uint32_t *table = a.tables + b * DEFLATE_TABLE_WORDS;
        table[t] = huff_entry(length, first_code, t);
        if (t == 0) table[DEFLATE_EOB] = huff_entry(length, first_code, DEFLATE_EOB);
        const uint32_t bits = wave_sum(freq[t] * length[t]);
        if (lane == 0) wbits[wave] = bits;
        wg_sync();
        if (t == 0) {
            DeflateBlock blk;
            blk.code_bits = wbits[0] + wbits[1] + wbits[2] + wbits[3] + length[DEFLATE_EOB];
            const uint32_t huffman = deflate_huffman_bytes(blk.code_bits, it.last);
            blk.huffman = huffman < 5u + it.len ? 1u : 0u;
            blk.bytes = blk.huffman ? huffman : 5u + it.len;
            blk.before = 0u;
            a.blocks[b] = blk;
        }
        wg_sync();                               // (the next item writes the LDS this one read)
    }
}

// The sum: a work item is a measured file.
__global__ __launch_bounds__(64 * COPY_WAVES) void deflate_sum_kernel(DeflateArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t entries = a.p.head->entries, total = a.p.head->blocks;
    const CopyWave wv = copy_wave();
    for (int64_t d = wv.me; d < entries; d += wv.waves) {
        DeflateSource f;
        uint32_t stream = 0u;                    // (a file's blocks are at most the stored ones: below 2^31 + 2^20)
        if (deflate_source(a, d, f) && f.first_block + f.blocks <= total) {
            for (unsigned i0 = 0; i0 < f.blocks; i0 += 64u) {
                const unsigned i = i0 + (unsigned)lane;
                const bool in = i < f.blocks;
                DeflateBlock *blk = a.blocks + f.first_block + (in ? i : 0u);
                const uint32_t x = in ? blk->bytes : 0u;
                const uint32_t inc = wave_inclusive_sum(x);
                if (in) blk->before = stream + inc - x;
                stream += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
            }
        }
        if (lane == 0) a.stream[d] = stream;
    }
}

// The place: png_plan_kernel over the measured entries' actual rooms.
__global__ __launch_bounds__(T) void deflate_place_kernel(DeflateArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wsum[1][PLAN_WAVES], wend[1][PLAN_WAVES];
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];
    const int64_t n = a.p.head->entries;
    int64_t byte_base = 0, used = 0;
    int64_t written = 0, skipped = 0, no_room = 0, invalid = 0;
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int64_t c = t0 + threadIdx.x, cc = c < n ? c : n - 1;
        const bool live = c < n;
        DeflateSource f;
        const bool writable = deflate_source(a, cc, f) && live;
        const int32_t source_status = a.p.level_dir[cc].status;
        const int64_t bytes = writable ? deflate_file_bytes(a.stream[cc]) : 0;
        const int64_t take[1] = {writable ? png_room(bytes) : 0};
        const TileScan<1> scan = tile_scan(take, wsum, lane, wave);
        const int64_t first_byte = byte_base + scan.before[0];
        const bool fits = writable && first_byte + take[0] <= a.p.png_bytes;
        const bool skip = live && source_status != RO_UNIT_WRITTEN;
        const bool is[PLAN_CLASSES] = {fits, skip, writable && !fits, live && !writable && !skip};
        const int64_t end[1] = {first_byte + take[0]};
        const TileCount<1> count = tile_count(is, end, wcnt, wend, lane, wave);
        written += count.total[0];
        skipped += count.total[1];
        no_room += count.total[2];
        invalid += count.total[3];
        used = count.end[0] > used ? count.end[0] : used;
        if (live) {
            const int status = writable ? (fits ? RO_UNIT_WRITTEN : RO_UNIT_NO_ROOM) : (skip ? RO_UNIT_SKIPPED : RO_UNIT_INVALID);
            int64_t *out = reinterpret_cast<int64_t *>(a.p.png_dir + c);        // ro_fits_unit_t, word by word
            out[0] = fits ? first_byte : 0;
            out[1] = bytes;
            out[2] = writable ? f.naxis2 : 0;
            out[3] = two_int32(writable ? (int32_t)f.naxis1 : 0, status);
        }
        byte_base += scan.total[0];
    }
    if (threadIdx.x == 0) png_store_summary(a.p.summary, n, written, skipped, no_room, invalid, used, byte_base);
}

// a written file as the place left it, checked once more against the buffers before anything of it is touched
struct DeflateFile {
    char *file;                    // file byte 0
    uint32_t stream;               // bytes of its blocks
    uint32_t idat;
    int64_t bytes;
};

__device__ __forceinline__ bool deflate_file(const DeflateArgs &a, int64_t d, const DeflateSource &s, DeflateFile &f)
{
    const ro_fits_unit_t *u = a.p.png_dir + d;
    const int64_t offset = u->offset, stream = a.stream[d], total = a.p.head->blocks;
    const int64_t bytes = deflate_file_bytes(stream);
    if (u->status != RO_UNIT_WRITTEN || stream < 0 || stream > (int64_t)s.blocks * PNG_PITCH || offset < 0 ||
        offset % RO_PNG_ALIGN != 0 || offset > a.p.png_bytes || png_room(bytes) > a.p.png_bytes - offset ||
        s.first_block + s.blocks > total)
        return false;
    f.file = a.p.png + offset;
    f.stream = (uint32_t)stream;
    f.idat = (uint32_t)deflate_idat(stream);
    f.bytes = bytes;
    return true;
}

// `bits` bits of value (its lowest first) at bit `at` of the staged block: an OR into one word or two
__device__ __forceinline__ void stage_bits(uint32_t *stage, uint32_t at, uint32_t value)
{
    const uint32_t w = at >> 5, sh = at & 31u;
    if (value << sh) atomicOr(&stage[w], value << sh);
    if (sh && (value >> (32u - sh))) atomicOr(&stage[w + 1u], value >> (32u - sh));
}

// what raw bytes i ... i + n - 1 of a block of len add to the Adler sums: their sum, and each times the raw bytes from it to
// the block's end
__device__ __forceinline__ void adler_word(unsigned len, unsigned i, unsigned v, uint32_t &sa, uint64_t &sb)
{
    const unsigned b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
    const unsigned sum = b0 + b1 + b2 + b3;      // (bytes behind the block's end are zeros)
    sa += sum;
    sb += (uint64_t)((len - i) * sum - (b1 + 2u * b2 + 3u * b3));
}

// The emit: a work item is a block of a measured entry; those of written files are taken.
__global__ __launch_bounds__(T) void deflate_emit_kernel(DeflateArgs a)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t total = a.p.head->blocks, entries = a.p.head->entries;
    __shared__ PngTables tab;
    __shared__ uint32_t stage[STAGE_WORDS];
    __shared__ uint32_t code[DEFLATE_TABLE_WORDS];
    __shared__ uint32_t red[PLAN_WAVES][4];      // the waves' CRC states, Adler sums and bits
    for (int i = t; i < (int)(sizeof(PngTables) / 4); i += T)
        reinterpret_cast<uint32_t *>(&tab)[i] = reinterpret_cast<const uint32_t *>(&TABLES)[i];
    wg_sync();
    for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
        DeflateSource src;
        DeflateItem it;
        DeflateFile f;
        if (!deflate_item(a, entries, b, src, it) || !deflate_file(a, it.d, src, f)) continue;
        const DeflateBlock blk = a.blocks[b];
        const unsigned n = blk.bytes, len = it.len;
        // (the measure's figures once more: the block lies inside its file's stream and inside the stage)
        if (n < 5u || n > (unsigned)PNG_PITCH || blk.before > f.stream || n > f.stream - blk.before) continue;
        const unsigned at = (unsigned)PNG_HEAD + blk.before;                     // the block's first byte in the file
        const unsigned p0 = at & 3u, np = p0 + n;                               // ... in its word; the staged bytes
        const unsigned words_all = (np + 3u) >> 2, full = np >> 2;
        char *base = f.file + (at - p0);                                        // the file's word the stage starts at
        for (unsigned j = (unsigned)t; j < words_all + 1u; j += (unsigned)T) stage[j] = 0u;
        if (blk.huffman) {
            code[t] = a.tables[b * DEFLATE_TABLE_WORDS + t];
            if (t == 0) code[DEFLATE_EOB] = a.tables[b * DEFLATE_TABLE_WORDS + DEFLATE_EOB];
        }
        wg_sync();
        uint32_t sa = 0u;
        uint64_t sb = 0u;
        if (blk.huffman) {
            // the header: the 74 bits by three lanes, a four-bit length by every lane
            const uint32_t head = 8u * p0;
            if (t < 3) stage_bits(stage, head + 32u * (unsigned)t, deflate_prefix_word(t, it.last));
            stage_bits(stage, head + DEFLATE_PREFIX_BITS + 4u * (unsigned)t, __brev(code[t] >> 16) >> 28);
            if (t == 0) stage_bits(stage, head + DEFLATE_PREFIX_BITS + 4u * DEFLATE_EOB, __brev(code[DEFLATE_EOB] >> 16) >> 28);
            // the lane's run of raw bytes, whole words of them
            const unsigned run = (((len + (unsigned)T - 1u) / (unsigned)T) + 3u) & ~3u;
            const unsigned first = run * (unsigned)t, mine = first < len ? (len - first < run ? len - first : run) : 0u;
            uint32_t bits = 0u;
            for (unsigned i = 0; i < mine; i += 4u) {
                unsigned m;
                const unsigned v = block_word(src, it.r0, len, first + i, m);
                adler_word(len, first + i, v, sa, sb);
#pragma unroll
                for (unsigned q = 0; q < 4u; ++q) bits += q < m ? code[(v >> (8u * q)) & 0xffu] >> 16 : 0u;
            }
            const uint32_t inc = wave_inclusive_sum(bits);
            if (lane == 63) red[wave][3] = inc;
            wg_sync();
            uint32_t pos = head + DEFLATE_HEAD_BITS + inc - bits;
#pragma unroll
            for (int v = 0; v < PLAN_WAVES; ++v) pos += v < wave ? red[v][3] : 0u;
            // the codes, a word at a time: the lane's first and last word are shared with its neighbours
            uint64_t acc = 0u;
            uint32_t held = pos & 31u, w = pos >> 5;
            for (unsigned i = 0; i < mine; i += 4u) {
                unsigned m;
                const unsigned v = block_word(src, it.r0, len, first + i, m);
#pragma unroll
                for (unsigned q = 0; q < 4u; ++q) {
                    const uint32_t c = q < m ? code[(v >> (8u * q)) & 0xffu] : 0u;
                    acc |= (uint64_t)(c & 0xffffu) << held;
                    held += c >> 16;
                    if (held >= 32u) {
                        if ((uint32_t)acc) atomicOr(&stage[w], (uint32_t)acc);
                        acc >>= 32;
                        held -= 32u;
                        w += 1u;
                    }
                }
            }
            if (t == T - 1) {
                // end-of-block behind the last lane's codes (lanes without a run stand where the codes end)
                const uint32_t c = code[DEFLATE_EOB];
                acc |= (uint64_t)(c & 0xffffu) << held;
                held += c >> 16;
            }
            if ((uint32_t)acc) atomicOr(&stage[w], (uint32_t)acc);
            if ((uint32_t)(acc >> 32)) atomicOr(&stage[w + 1u], (uint32_t)(acc >> 32));
            // the ending of a block that is not the last: its zeros are there; FF FF are the block's last two bytes
            if (t == 0 && !it.last) stage_bits(stage, 8u * (np - 2u), 0xffffu);
        } else {
            const uint32_t head = 8u * p0, nlen = ~len & 0xffffu;
            if (t == 0) {
                stage_bits(stage, head, (it.last ? 1u : 0u) | (len << 8) | ((nlen & 0xffu) << 24));
                stage_bits(stage, head + 32u, nlen >> 8);
            }
            const unsigned words = (len + 3u) >> 2;
            for (unsigned j = (unsigned)t; j < words; j += (unsigned)T) {
                unsigned m;
                const unsigned v = block_word(src, it.r0, len, 4u * j, m);
                adler_word(len, 4u * j, v, sa, sb);
                stage_bits(stage, head + 40u + 32u * j, v);
            }
        }
        wg_sync();
        // the stage to the file, and its CRC: the lane's words from the lowest address on, word full - 1 - t - 256 m, so
        // that every lane's last word lies 4 t bytes in front of the last whole word's end (the zeros in front of the
        // block in its first word, like words in front of the stage, are zeros a remainder does not see)
        for (unsigned j = (unsigned)t; j < words_all; j += (unsigned)T) {
            const unsigned lo = 4u * j < p0 ? p0 : 4u * j, hi = 4u * j + 4u > np ? np : 4u * j + 4u;
            const uint32_t v = stage[j];
            if (hi - lo == 4u) reinterpret_cast<uint32_t *>(base)[j] = v;
            else
                for (unsigned q = lo; q < hi; ++q) base[q] = (char)((v >> (8u * (q & 3u))) & 0xffu);
        }
        const int steps = ((int)full + T - 1) / T;
        uint32_t crc = 0u;
        for (int m = steps - 1; m >= 0; --m) {
            const int s = (int)full - 1 - t - T * m;
            const uint32_t v = s >= 0 ? stage[s] : 0u;
            crc = m > 0 ? crc_word(tab.gap, crc ^ v) : crc_word(tab.byte, crc ^ v);
        }
        crc = crc_mul(crc, tab.lane[t]);
        crc = wave_xor(crc);
        sa = wave_sum(sa % ADLER_MOD);
        const uint32_t sbm = wave_sum((uint32_t)(sb % ADLER_MOD));
        if (lane == 0) {
            red[wave][0] = crc;
            red[wave][1] = sa;
            red[wave][2] = sbm;
        }
        wg_sync();
        if (wave == 0) {
            // IDAT bytes behind this block: the lower half wave raises x to them, the upper one to them and the block
            const unsigned behind = f.idat - (2u + blk.before + n);
            const uint32_t power = wave_xpow8(tab.x2n, lane < 32 ? behind : behind + n, lane);
            const uint32_t power_block = (uint32_t)__shfl((int)power, 32);
            if (lane == 0) {
                uint32_t c, A, B;
                png_fold(red, c, A, B);
                for (unsigned q = 4u * full; q < np; ++q) c = crc_byte(tab, c, (stage[q >> 2] >> (8u * (q & 3u))) & 0xffu);
                // what stands in front of block 0 in the chunk's CRC: the chunk type and 78 01
                uint32_t pre = 0u;
                if (it.k == 0)
                    for (int i = 37; i < (int)PNG_HEAD; ++i) pre = crc_byte(tab, pre, png_head_byte(i, 0u, 0u, 0u, 0u, false, 0u));
                a.p.parts[b] = png_part(c, A, B, pre, power, power_block, src.raw - it.r0 - len);
            }
        } else if (wave == 1 && it.k == 0) {
            // the file's head, by another wave: 43 bytes, most of them constants
            uint32_t c = 0xffffffffu;
            for (int i = 12; i < 29; ++i) c = crc_byte(tab, c, png_head_byte(i, src.naxis1, (uint32_t)src.naxis2, 0u, 0u, false, 0u));
            if (lane < (int)PNG_HEAD) f.file[lane] = (char)png_head_byte(lane, src.naxis1, (uint32_t)src.naxis2, ~c, f.idat, false, 0u);
        }
        wg_sync();                               // (the next item writes the LDS this one read)
    }
}

// The finish: a work item is a file.
__global__ __launch_bounds__(64 * COPY_WAVES) void deflate_finish_kernel(DeflateArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t entries = a.p.head->entries;
    const CopyWave wv = copy_wave();
    for (int64_t d = wv.me; d < entries; d += wv.waves) {
        DeflateSource src;
        DeflateFile f;
        if (!deflate_source(a, d, src) || !deflate_file(a, d, src, f)) continue;
        uint32_t c = 0u, A = 0u, B = 0u;
        for (unsigned i = (unsigned)lane; i < src.blocks; i += 64u) {
            const PngPart part = a.p.parts[src.first_block + i];
            c ^= part.crc;
            A = (A + part.a) % ADLER_MOD;
            B = (B + part.b) % ADLER_MOD;
        }
        c = wave_xor(c);
        A = (1u + wave_sum(A)) % ADLER_MOD;
        B = (src.raw % ADLER_MOD + wave_sum(B)) % ADLER_MOD;
        const uint32_t adler = (B << 16) | A;
        // the chunk's CRC runs over its type and its data, the Adler-32 last
        const uint32_t power = wave_xpow8(TABLES.x2n, 4u + f.idat, lane);
        uint32_t tail = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) tail = crc_byte_plain(tail, png_tail_byte(i, adler, 0u));
        const uint32_t crc = c ^ tail ^ crc_mul(0xffffffffu, power) ^ 0xffffffffu;
        const int64_t end = f.bytes - PNG_TAIL;
        if (lane < PNG_TAIL + (int)(png_room(f.bytes) - f.bytes))
            f.file[end + lane] = lane < PNG_TAIL ? (char)png_tail_byte(lane, adler, crc) : (char)0;
    }
}

}  // namespace

size_t deflate_scratch_bytes(int64_t dir_capacity, int64_t levels_bytes)
{
    const size_t blocks = (size_t)deflate_max_blocks(dir_capacity, levels_bytes);
    return sizeof(PngPlanHead) + blocks * (sizeof(PngPart) + sizeof(DeflateBlock) + DEFLATE_TABLE_WORDS * sizeof(uint32_t)) +
           (size_t)dir_capacity * 2 * sizeof(int64_t);
}

void deflate_scratch_layout(DeflateArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.p.max_blocks = deflate_max_blocks(a.p.dir_capacity, a.p.levels_bytes);
    const size_t blocks = (size_t)a.p.max_blocks, entries = (size_t)a.p.dir_capacity;
    a.p.head = reinterpret_cast<PngPlanHead *>(p);
    p += sizeof(PngPlanHead);
    a.p.parts = reinterpret_cast<PngPart *>(p);
    p += blocks * sizeof(PngPart);
    a.blocks = reinterpret_cast<DeflateBlock *>(p);
    p += blocks * sizeof(DeflateBlock);
    a.p.first_block = reinterpret_cast<int64_t *>(p);
    p += entries * sizeof(int64_t);
    a.stream = reinterpret_cast<int64_t *>(p);
    p += entries * sizeof(int64_t);
    a.tables = reinterpret_cast<uint32_t *>(p);
}

hipError_t launch_levels_png_deflate(const DeflateArgs &a, int cus, hipStream_t s)
{
    const PngArgs &p = a.p;
    if (!png_args_valid(p) || !a.stream || !a.blocks || !a.tables || p.max_blocks != deflate_max_blocks(p.dir_capacity, p.levels_bytes))
        return hipErrorInvalidValue;
    // the work is known on the device only, but it is at most the blocks of the levels and the entries of the directory
    const unsigned block_grid = png_grid_for(copy_grid(cus), p.max_blocks, 1);
    const unsigned file_grid = png_grid_for(copy_grid(cus), p.dir_capacity, COPY_WAVES);
    hipLaunchKernelGGL(deflate_want_kernel, dim3(1), dim3(T), 0, s, a);
    hipLaunchKernelGGL(deflate_measure_kernel, dim3(block_grid), dim3(T), 0, s, a);
    hipLaunchKernelGGL(deflate_sum_kernel, dim3(file_grid), dim3(64 * COPY_WAVES), 0, s, a);
    hipLaunchKernelGGL(deflate_place_kernel, dim3(1), dim3(T), 0, s, a);
    hipLaunchKernelGGL(deflate_emit_kernel, dim3(block_grid), dim3(T), 0, s, a);
    hipLaunchKernelGGL(deflate_finish_kernel, dim3(file_grid), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
