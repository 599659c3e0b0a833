// sanitize_png_deflate_host.cpp -- ro_levels_png_deflate_host and ro_levels_png_host, the two twins over the host's one walk
// and one file writer, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program over the tests' shape
// table times a content table and the room cases, every buffer allocated at its exact size so that a byte read or written
// past one is seen.  Where every block stays stored (random levels, at every shape but 1 x 70000, whose raw bytes are half
// filter bytes) the two calls' files are held to the same bytes.  Host code only: it needs no GPU and is not part of the suite.
//   cd radio-observer_amd/csrc && hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize -Xarch_host
//     -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o /tmp/sanitize_png_deflate_host
//     ../../tools/png/sanitize_png_deflate_host.cpp *.hip *.cpp && /tmp/sanitize_png_deflate_host
// Prints one line per case and "ok"; a finding aborts the run with the sanitizer's report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ro_stft.h"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ull;
uint32_t next_u32()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

std::vector<unsigned char> pixels_of(int content, int64_t w, int64_t h)
{
    std::vector<unsigned char> px((size_t)(w * h));
    const int64_t n = w * h;
    for (int64_t i = 0; i < n; ++i) {
        unsigned char v = 0;
        if (content == 0) v = (unsigned char)next_u32();                                     // random
        else if (content == 1) v = 0xff;                                                     // ones
        else if (content == 2) v = 0;                                                        // zeros
        else if (content == 3) {                                                             // noise: a bell around 150
            unsigned sum = 0;
            for (int k = 0; k < 6; ++k) sum += next_u32() & 63u;
            v = (unsigned char)(sum * 255u / 378u);
            if (next_u32() % 4001u == 0) v = (unsigned char)next_u32();                      // ... with rare far values
        } else if (content == 4) {                                                           // fib: value k stands F(k) times
            int64_t at = i % 65000, f0 = 1, f1 = 2;
            v = 1;
            while (at >= f0) {
                at -= f0;
                const int64_t f2 = f0 + f1;
                f0 = f1;
                f1 = f2;
                v += 1;
            }
        } else v = i < n / 2 ? (unsigned char)next_u32() : 0;                                // mixed
        px[(size_t)i] = v;
    }
    return px;
}

struct Run {
    std::vector<ro_fits_unit_t> dir;
    std::vector<unsigned char> png;
    ro_unit_summary_t summary;
};

// exact-size heap buffers for every argument; deflate: ro_levels_png_deflate_host, else ro_levels_png_host
Run call(bool deflate, const std::vector<ro_fits_unit_t> &level_dir, int64_t entries, const std::vector<unsigned char> &levels,
         int64_t room)
{
    Run r;
    r.dir.resize(level_dir.size());
    r.png.resize((size_t)room);
    ro_unit_summary_t level_summary{};
    level_summary.entries = entries;
    const int rc = (deflate ? ro_levels_png_deflate_host : ro_levels_png_host)(
        level_dir.empty() ? nullptr : level_dir.data(), (int64_t)level_dir.size(), &level_summary,
        levels.empty() ? nullptr : levels.data(), (int64_t)levels.size(),
        r.dir.empty() ? reinterpret_cast<ro_fits_unit_t *>(&r.summary) : r.dir.data(), room ? r.png.data() : nullptr, room, &r.summary);
    if (rc != RO_OK) {
        std::printf("refused: %s\n", ro_last_error());
        std::exit(1);
    }
    return r;
}

}  // namespace

int main()
{
    const int64_t shapes[][2] = {{1, 1}, {4368, 15}, {255, 256}, {4368, 30}, {65534, 2}, {1, 70000}, {615, 352}};
    const char *names[] = {"random", "ones", "zeros", "noise", "fib", "mixed"};
    for (const auto &shape : shapes)
        for (int content = 0; content < 6; ++content) {
            const int64_t w = shape[0], h = shape[1];
            // the image behind a one-pixel one, a skipped and an invalid entry; the levels end with the image's last pixel
            std::vector<unsigned char> levels((size_t)RO_LEVEL_BLOCK, 7);
            const std::vector<unsigned char> px = pixels_of(content, w, h);
            levels.insert(levels.end(), px.begin(), px.end());
            std::vector<ro_fits_unit_t> dir(4);
            dir[0] = {0, 1, 1, 1, RO_UNIT_WRITTEN};
            dir[1] = {0, 0, 0, 0, RO_UNIT_SKIPPED};
            dir[2] = {RO_LEVEL_BLOCK, w * h + 1, h, (int32_t)w, RO_UNIT_WRITTEN};
            dir[3] = {RO_LEVEL_BLOCK, w * h, h, (int32_t)w, RO_UNIT_WRITTEN};
            const Run sizing = call(true, dir, 4, levels, 0);
            const int64_t need = sizing.summary.needed_bytes;
            const Run full = call(true, dir, 9, levels, need), again = call(true, dir, 4, levels, need),
                      tight = call(true, dir, 4, levels, need - 1);
            // the stored call over the same arguments: its room is arithmetic
            const int64_t stored_need = call(false, dir, 4, levels, 0).summary.needed_bytes;
            const Run stored = call(false, dir, 9, levels, stored_need), stored_tight = call(false, dir, 4, levels, stored_need - 1);
            const bool all_stored = content == 0 && !(w == 1 && h == 70000);
            const bool ok = stored.summary.written == 2 && stored.summary.units_bytes == stored_need && stored_need >= need &&
                            stored.dir[3].bytes == ro_png_bytes((int32_t)w, h) && stored_tight.summary.written == 1 &&
                            stored_tight.summary.no_room == 1 &&
                            std::memcmp(stored_tight.png.data(), stored.png.data(), (size_t)stored_tight.summary.units_bytes) == 0 &&
                            (!all_stored || (stored.png == full.png &&
                                             std::memcmp(stored.dir.data(), full.dir.data(), stored.dir.size() * sizeof(ro_fits_unit_t)) == 0)) &&
                            sizing.summary.written == 0 && sizing.summary.no_room == 2 && sizing.summary.skipped == 1 &&
                            sizing.summary.invalid == 1 && full.summary.written == 2 && full.summary.units_bytes == need &&
                            full.png == again.png && tight.summary.written == 1 && tight.summary.no_room == 1 &&
                            full.dir[3].bytes == sizing.dir[3].bytes && full.dir[3].bytes <= ro_png_bytes((int32_t)w, h) &&
                            std::memcmp(tight.png.data(), full.png.data(), tight.png.size() ? (size_t)tight.summary.units_bytes : 0) == 0;
            std::printf("%5lld x %5lld %-6s  %8lld bytes of at most %8lld  %s%s\n", (long long)w, (long long)h, names[content],
                        (long long)full.dir[3].bytes, (long long)ro_png_bytes((int32_t)w, h), all_stored ? "the stored call's bytes  " : "",
                        ok ? "" : "MISMATCH");
            if (!ok) return 1;
        }
    if (call(true, {}, 0, {}, 0).summary.entries != 0 || call(false, {}, 0, {}, 0).summary.entries != 0) return 1;
    std::printf("ok\n");
    return 0;
}
