// ro_png.hip -- the preview files on the device: every level image of a level directory (what
// ro_stft_snapshot_levels_resident leaves, or ro_periodic_level_dir makes of a periodic plan) as a complete PNG -- 8 bit
// grey, a filter byte 0 in front of every scanline, the zlib stream in stored deflate blocks of 65535 raw bytes, its
// Adler-32, the IDAT CRC-32, IEND -- each file at a multiple of 16 bytes of one buffer, with a directory.
// include/ro_stft.h states the file to the byte and the entry rules; ro_png.h has the file's arithmetic and the checksum
// constants.  Nothing is remembered from call to call and the levels and their directory are only read.
//
// Plain launches; no workgroup waits for another one of its launch, no atomics, and every checksum is integer arithmetic
// whose result does not depend on the order of its terms, so the same input gives the same bytes:
//   png_plan_kernel    the plan of ro_pack_plan.h over the level directory: what is scanned are the writable entries'
//                      rooms (a file's bytes rounded up to 16) and their stored blocks.  It writes the directory (entry d
//                      is level entry d), the summary and the plan (ro_png.h)
//   png_blocks_kernel  a workgroup takes a stored block: lanes on consecutive words of it, a lane on every 256th word.  It
//                      gathers the raw bytes (the filter byte where a scanline starts), stores them behind the block's
//                      header, and leaves what the block adds to the file's two checksums in scratch (PngPart): a lane's
//                      CRC runs over its own words with a table that steps over the 1020 bytes between them, x^(32 lane)
//                      brings it to the block's end, the lanes' states add up in LDS, and one multiplication takes the
//                      block to the end of the chunk.  Block 0's workgroup writes the file's first 48 bytes too
//   png_finish_kernel  a wave takes a file: adds its blocks' parts, writes the Adler-32, the IDAT CRC, IEND and the zeros
//                      up to the next multiple of 16
// Every level byte is read once and a byte is written per raw byte.  What these kernels and ro_png_deflate.hip's do the same
// way once per entry or per block is ro_png_crc_device.h's; the launchers' common checks and grids are ro_png.h's.
#include "ro_pack_plan.h"
#include "ro_png.h"
#include "ro_png_crc_device.h"

namespace ro {

namespace {

constexpr int T = RO_PNG_TILE;
static_assert(T == PLAN_TILE && T == PNG_LANES, "one entry per lane, four waves");
static_assert(sizeof(ro_fits_unit_t) == 32 && offsetof(ro_fits_unit_t, naxis1) == 24 && offsetof(ro_fits_unit_t, status) == 28 &&
                  sizeof(ro_unit_summary_t) == 64 && sizeof(PngPart) == 16,
              "png_plan_kernel reads and writes an entry as its four words");
static_assert(PNG_DATA % RO_PNG_ALIGN == 0 && PNG_PITCH % 4 == 0, "a block's raw bytes start at a word of the file");

__device__ const PngTables TABLES = make_png_tables();

// The plan.  An entry FITS when the rooms up to and including its own are at most png_bytes.
__global__ __launch_bounds__(T) void png_plan_kernel(PngArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    __shared__ int64_t wsum[2][PLAN_WAVES], wend[2][PLAN_WAVES];
    __shared__ int wcnt[PLAN_CLASSES][PLAN_WAVES];    // written, skipped, no room, invalid of each wave
    int64_t n = *a.entries;
    n = n < 0 ? 0 : (n > a.dir_capacity ? a.dir_capacity : n);
    int64_t byte_base = 0, block_base = 0;       // rooms and blocks of the writable entries in front of the tile
    int64_t used = 0, used_blocks = 0;           // ... of the written ones: where the last written file ends
    int64_t written = 0, skipped = 0, no_room = 0, invalid = 0;
#pragma unroll 1
    for (int64_t t0 = 0; t0 < n; t0 += T) {
        const int64_t c = t0 + threadIdx.x;
        // (lanes past the last entry read it once more and take no part: no guarded load of a struct)
        const PngWant w = png_want_entry(a.level_dir, c < n ? c : n - 1, a.levels_bytes);
        const bool live = c < n;
        const bool writable = live && w.status == RO_UNIT_WRITTEN;
        const int64_t take[2] = {writable ? png_room(w.bytes) : 0, writable ? w.blocks : 0};
        const TileScan<2> scan = tile_scan(take, wsum, lane, wave);
        const int64_t first_byte = byte_base + scan.before[0], first_b = block_base + scan.before[1];
        const bool fits = writable && first_byte + take[0] <= a.png_bytes;
        const bool is[PLAN_CLASSES] = {fits, live && w.status == RO_UNIT_SKIPPED, writable && !fits,
                                       live && w.status == RO_UNIT_INVALID};
        const int64_t end[2] = {first_byte + take[0], first_b + take[1]};
        const TileCount<2> count = tile_count(is, end, wcnt, wend, lane, wave);
        written += count.total[0];
        skipped += count.total[1];
        no_room += count.total[2];
        invalid += count.total[3];
        used = count.end[0] > used ? count.end[0] : used;
        used_blocks = count.end[1] > used_blocks ? count.end[1] : used_blocks;
        if (live) {
            const int status = writable ? (fits ? RO_UNIT_WRITTEN : RO_UNIT_NO_ROOM) : w.status;
            int64_t *out = reinterpret_cast<int64_t *>(a.png_dir + c);          // ro_fits_unit_t, word by word
            out[0] = fits ? first_byte : 0;                                                               // offset
            out[1] = writable ? w.bytes : 0;                                                              // bytes
            out[2] = writable ? w.naxis2 : 0;                                                             // naxis2
            out[3] = two_int32(writable ? w.naxis1 : 0, status);                                          // naxis1, status
            a.first_block[c] = first_b;
        }
        byte_base += scan.total[0];
        block_base += scan.total[1];
    }
    if (threadIdx.x == 0) {
        png_store_summary(a.summary, n, written, skipped, no_room, invalid, used, byte_base);
        PngPlanHead head;
        head.entries = n;
        head.blocks = used_blocks < a.max_blocks ? used_blocks : a.max_blocks;     // (files side by side have no more)
        *a.head = head;
    }
}

// a written file as the plan left it, checked once more against the buffers before anything of it is touched
struct PngFile {
    const unsigned char *src;      // level of pixel 0
    char *file;                    // file byte 0
    unsigned naxis1, naxis2, raw, blocks, idat;
    int64_t bytes;                 // the file's
    int64_t first_block;
};

__device__ __forceinline__ bool png_file(const PngArgs &a, int64_t d, PngFile &f)
{
    const ro_fits_unit_t *u = a.png_dir + d;
    const int64_t offset = u->offset, naxis2 = u->naxis2, source = a.level_dir[d].offset, first = a.first_block[d];
    const int32_t naxis1 = u->naxis1;
    int64_t raw, blocks, idat;
    if (u->status != RO_UNIT_WRITTEN || !png_shape(naxis1, naxis2, &raw, &blocks, &idat)) return false;
    const int64_t bytes = png_file_bytes(naxis1, naxis2), pixels = (int64_t)naxis1 * naxis2;
    if (offset < 0 || offset % RO_PNG_ALIGN != 0 || offset > a.png_bytes || png_room(bytes) > a.png_bytes - offset || source < 0 ||
        source > a.levels_bytes || pixels > a.levels_bytes - source || first < 0 || first > a.max_blocks ||
        blocks > a.max_blocks - first)
        return false;
    f.src = a.levels + source;
    f.file = a.png + offset;
    f.naxis1 = (unsigned)naxis1;
    f.naxis2 = (unsigned)naxis2;
    f.raw = (unsigned)raw;
    f.blocks = (unsigned)blocks;
    f.idat = (unsigned)idat;
    f.bytes = bytes;
    f.first_block = first;
    return true;
}

constexpr int WORDS_AHEAD = 8;                   // words a lane gathers before it looks at the first

// The blocks: a work item is a stored block, a workgroup takes it.
__global__ __launch_bounds__(T) void png_blocks_kernel(PngArgs a)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t total = a.head->blocks, entries = a.head->entries;
    if ((int64_t)blockIdx.x >= total) return;
    __shared__ PngTables tab;
    __shared__ uint32_t red[2][PLAN_WAVES][3];   // the waves' states and sums of this item and of the one before
    for (int i = t; i < (int)(sizeof(PngTables) / 4); i += T)
        reinterpret_cast<uint32_t *>(&tab)[i] = reinterpret_cast<const uint32_t *>(&TABLES)[i];
    wg_sync();
    int turn = 0;
    for (int64_t b = blockIdx.x; b < total; b += gridDim.x) {
        const int64_t d = plan_entry(a.first_block, entries, b);
        PngFile f;
        if (d < 0 || !png_file(a, d, f)) continue;
        const int64_t k64 = b - f.first_block;
        if (k64 >= f.blocks) continue;
        const unsigned k = (unsigned)k64;
        const unsigned r0 = k * (unsigned)PNG_STORED;                            // the block's first raw byte
        const unsigned len = f.raw - r0 < PNG_STORED ? f.raw - r0 : (unsigned)PNG_STORED;
        const bool last = k + 1 == f.blocks;
        char *block = f.file + PNG_HEAD + (int64_t)k * PNG_PITCH;                // its header
        unsigned *__restrict__ out = reinterpret_cast<unsigned *>(block + 5);    // its raw bytes
        const int full = (int)(len >> 2);                                        // whole words of it
        const int steps = (full + T - 1) / T;
        // the lane's words from the lowest address on: word full - 1 - t - 256 m for m = steps - 1 ... 0, so that every
        // lane's last word lies 4 t bytes in front of the last whole word's end (words in front of the block are zeros,
        // which a remainder does not see)
        uint32_t crc = 0u, sa = 0u;
        uint64_t sb = 0u;
        for (int q0 = 0; q0 < steps; q0 += WORDS_AHEAD) {
            unsigned word[WORDS_AHEAD];
#pragma unroll
            for (int j = 0; j < WORDS_AHEAD; ++j) {
                const int m = steps - 1 - q0 - j;
                const int s = m >= 0 ? full - 1 - t - T * m : -1;
                word[j] = raw_word(f.src, f.naxis1, r0 + 4u * (unsigned)(s > 0 ? s : 0));
            }
#pragma unroll
            for (int j = 0; j < WORDS_AHEAD; ++j) {
                const int m = steps - 1 - q0 - j;
                if (m < 0) continue;
                const int s = full - 1 - t - T * m;
                const unsigned v = s >= 0 ? word[j] : 0u;
                if (s >= 0) out[s] = v;
                const unsigned b0 = v & 0xffu, b1 = (v >> 8) & 0xffu, b2 = (v >> 16) & 0xffu, b3 = v >> 24;
                const unsigned sum = b0 + b1 + b2 + b3;
                sa += sum;
                sb += (uint64_t)((len - 4u * (unsigned)(s > 0 ? s : 0)) * sum - (b1 + 2u * b2 + 3u * b3));
                crc = m > 0 ? crc_word(tab.gap, crc ^ v) : crc_word(tab.byte, crc ^ v);
            }
        }
        crc = crc_mul(crc, tab.lane[t]);
        crc = wave_xor(crc);
        sa = wave_sum(sa % ADLER_MOD);
        const uint32_t sbm = wave_sum((uint32_t)(sb % ADLER_MOD));
        if (lane == 0) {
            red[turn][wave][0] = crc;
            red[turn][wave][1] = sa;
            red[turn][wave][2] = sbm;
        }
        wg_sync();
        const bool final0 = f.blocks == 1;
        const unsigned len0 = f.raw < PNG_STORED ? f.raw : (unsigned)PNG_STORED;
        if (wave == 0) {
            // IDAT bytes behind this block: the lower half wave raises x to them, the upper one to them and the block
            const unsigned behind = f.idat - (2u + k * (unsigned)PNG_PITCH + 5u + len);
            const uint32_t power = wave_xpow8(tab.x2n, lane < 32 ? behind : behind + len, lane);
            const uint32_t power_block = (uint32_t)__shfl((int)power, 32);
            if (lane == 0) {
                uint32_t c, A, B;
                png_fold(red[turn], c, A, B);
                // the bytes behind the last whole word; a block that is not the last has three, and the word they
                // share with the next block's first header byte is written here
                unsigned word = 0u;
                for (unsigned i = 4u * (unsigned)full; i < len; ++i) {
                    const unsigned v = raw_byte(f.src, f.naxis1, r0 + i);
                    c = crc_byte(tab, c, v);
                    A += v;
                    B += (len - i) * v;
                    word |= v << (8 * (i & 3u));
                    if (last) block[5 + i] = (char)v;
                }
                if (!last) out[full] = word | (png_block_header_byte(0, k + 2 == f.blocks, 0u) << 24);
                // what stands in front of the raw bytes in the chunk's CRC: the header, and the chunk type and 78 01
                uint32_t pre = 0u;
                if (k == 0) {
                    for (int i = 37; i < (int)PNG_DATA; ++i) pre = crc_byte(tab, pre, png_head_byte(i, 0u, 0u, 0u, 0u, final0, len0));
                } else {
                    for (int i = 0; i < 5; ++i) pre = crc_byte(tab, pre, png_block_header_byte(i, last, len));
                    *reinterpret_cast<unsigned *>(block + 1) = len | ((~len & 0xffffu) << 16);               // LEN, ~LEN
                }
                a.parts[b] = png_part(c, A, B, pre, power, power_block, f.raw - r0 - len);
            }
        } else if (t == 64 && k == 0) {
            // the file's head, by one lane of another wave: 48 bytes, most of them constants
            uint32_t c = 0xffffffffu;
            for (int i = 12; i < 29; ++i) c = crc_byte(tab, c, png_head_byte(i, f.naxis1, f.naxis2, 0u, 0u, false, 0u));
            for (int i = 0; i < (int)PNG_DATA; ++i) f.file[i] = (char)png_head_byte(i, f.naxis1, f.naxis2, ~c, f.idat, final0, len0);
        }
        turn ^= 1;
    }
}

// The finish: a work item is a file.
__global__ __launch_bounds__(64 * COPY_WAVES) void png_finish_kernel(PngArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t entries = a.head->entries, total = a.head->blocks;
    const CopyWave wv = copy_wave();
    for (int64_t d = wv.me; d < entries; d += wv.waves) {
        PngFile f;
        if (!png_file(a, d, f) || f.first_block + f.blocks > total) continue;
        uint32_t c = 0u, A = 0u, B = 0u;
        for (unsigned i = (unsigned)lane; i < f.blocks; i += 64u) {
            const PngPart part = a.parts[f.first_block + i];
            c ^= part.crc;
            A = (A + part.a) % ADLER_MOD;
            B = (B + part.b) % ADLER_MOD;
        }
        c = wave_xor(c);
        A = (1u + wave_sum(A)) % ADLER_MOD;
        B = (f.raw % ADLER_MOD + wave_sum(B)) % ADLER_MOD;
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

size_t png_scratch_bytes(int64_t dir_capacity, int64_t png_bytes)
{
    return sizeof(PngPlanHead) + (size_t)png_max_blocks(dir_capacity, png_bytes) * sizeof(PngPart) +
           (size_t)dir_capacity * sizeof(int64_t);
}

void png_scratch_layout(PngArgs &a, void *scratch)
{
    char *p = static_cast<char *>(scratch);
    a.max_blocks = png_max_blocks(a.dir_capacity, a.png_bytes);
    a.head = reinterpret_cast<PngPlanHead *>(p);
    a.parts = reinterpret_cast<PngPart *>(p + sizeof(PngPlanHead));
    a.first_block = reinterpret_cast<int64_t *>(p + sizeof(PngPlanHead) + (size_t)a.max_blocks * sizeof(PngPart));
}

hipError_t launch_levels_png(const PngArgs &a, int cus, hipStream_t s)
{
    if (!png_args_valid(a) || a.max_blocks != png_max_blocks(a.dir_capacity, a.png_bytes)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(png_plan_kernel, dim3(1), dim3(T), 0, s, a);
    // the work is known on the device only, but it is at most the blocks of the room and the entries of the directory
    hipLaunchKernelGGL(png_blocks_kernel, dim3(png_grid_for(copy_grid(cus), a.max_blocks, 1)), dim3(T), 0, s, a);
    hipLaunchKernelGGL(png_finish_kernel, dim3(png_grid_for(copy_grid(cus), a.dir_capacity, COPY_WAVES)), dim3(64 * COPY_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
