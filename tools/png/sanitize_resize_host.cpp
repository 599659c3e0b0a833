// sanitize_resize_host.cpp -- ro_resize_plan and ro_levels_resize_host, the plan and the host twin of the resized previews,
// under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program over the tests' shape table times a content
// table and the room cases, every buffer -- the levels, the directories, the plan blob, the out levels -- allocated at its
// exact size so that a byte read or written past one is seen.  Host code only: it needs no GPU and is not part of the suite.
//   cd radio-observer_amd/csrc && hipcc -O1 -g --offload-arch=gfx950 -std=c++17 -fno-slp-vectorize -Xarch_host
//     -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -o /tmp/sanitize_resize_host
//     ../../tools/png/sanitize_resize_host.cpp *.hip *.cpp && /tmp/sanitize_resize_host
// Prints one line per case and "ok"; a finding aborts the run with the sanitizer's report.
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
    for (int64_t i = 0; i < w * h; ++i) {
        unsigned char v = 0;
        if (content == 0) v = (unsigned char)next_u32();                                     // random
        else if (content == 1) v = 0xff;                                                     // ones
        else if (content == 2) v = 0;                                                        // zeros
        else if (content == 3) v = ((i / w + i % w) & 1) ? 0xff : 0;                         // checker: both clamps
        else {                                                                               // a bell around 150
            unsigned sum = 0;
            for (int k = 0; k < 6; ++k) sum += next_u32() & 63u;
            v = (unsigned char)(sum * 255u / 378u);
        }
        px[(size_t)i] = v;
    }
    return px;
}

struct Run {
    std::vector<ro_fits_unit_t> dir;
    std::vector<unsigned char> out;
    ro_unit_summary_t summary;
    ro_resize_info_t info;
};

void must(int rc)
{
    if (rc != RO_OK) {
        std::printf("refused: %s\n", ro_last_error());
        std::exit(1);
    }
}

// the sizing form, the plan at its exact size, the resize into exactly `room` bytes
Run call(const std::vector<ro_fits_unit_t> &level_dir, int64_t entries, const std::vector<unsigned char> &levels, int32_t width, int64_t room)
{
    Run r;
    r.dir.resize(level_dir.size());
    r.out.resize((size_t)room);
    ro_unit_summary_t level_summary{};
    level_summary.entries = entries;
    ro_fits_unit_t *out_dir = r.dir.empty() ? reinterpret_cast<ro_fits_unit_t *>(&r.summary) : r.dir.data();
    const ro_fits_unit_t *dir = level_dir.empty() ? nullptr : level_dir.data();
    must(ro_resize_plan(dir, (int64_t)level_dir.size(), &level_summary, (int64_t)levels.size(), width, out_dir, room, &r.summary, nullptr, 0,
                        &r.info));
    std::vector<uint64_t> plan((size_t)(r.info.plan_bytes / 8));
    must(ro_resize_plan(dir, (int64_t)level_dir.size(), &level_summary, (int64_t)levels.size(), width, out_dir, room, &r.summary, plan.data(),
                        r.info.plan_bytes, &r.info));
    must(ro_levels_resize_host(&r.info, plan.data(), levels.empty() ? nullptr : levels.data(), (int64_t)levels.size(),
                               room ? r.out.data() : nullptr, room));
    return r;
}

}  // namespace

int main()
{
    const int64_t shapes[][3] = {{2, 2, 1},      {7, 5, 3},       {19, 40, 1},    {3, 300, 2},      {33, 100, 32},     {1000, 64, 999},
                                 {257, 131, 129}, {721, 9, 100},   {410, 37, 128}, {615, 352, 200},  {5120, 219, 1024}, {70000, 300, 256},
                                 {9, 2, 4},       {30, 7, 30}};
    const char *names[] = {"random", "ones", "zeros", "checker", "bell"};
    for (const auto &shape : shapes)
        for (int content = 0; content < 5; ++content) {
            const int64_t w = shape[0], h = shape[1];
            const int32_t width = (int32_t)shape[2];
            // the image behind a one-pixel one, a skipped and an invalid entry; the levels end with the image's last pixel
            std::vector<unsigned char> levels((size_t)RO_LEVEL_BLOCK, 7);
            const std::vector<unsigned char> px = pixels_of(content, w, h);
            levels.insert(levels.end(), px.begin(), px.end());
            std::vector<ro_fits_unit_t> dir(4);
            dir[0] = {0, 1, 1, 1, RO_UNIT_WRITTEN};
            dir[1] = {0, 0, 0, 0, RO_UNIT_SKIPPED};
            dir[2] = {RO_LEVEL_BLOCK, w * h + 1, h, (int32_t)w, RO_UNIT_WRITTEN};
            dir[3] = {RO_LEVEL_BLOCK, w * h, h, (int32_t)w, RO_UNIT_WRITTEN};
            int32_t w2 = 0;
            int64_t h2 = 0;
            must(ro_resize_shape((int32_t)w, h, width, &w2, &h2));
            const Run sizing = call(dir, 4, levels, width, 0);
            const int64_t need = sizing.summary.needed_bytes;
            const Run full = call(dir, 9, levels, width, need), again = call(dir, 4, levels, width, need);
            bool ok = full.out == again.out && full.summary.units_bytes == need && sizing.summary.written == 0;
            if (h2 == 0) ok = ok && full.summary.written == 1 && full.summary.skipped == 2 && full.summary.invalid == 1 && need == RO_LEVEL_BLOCK;
            else {
                const Run tight = call(dir, 4, levels, width, need - 1);
                ok = ok && full.summary.written == 2 && full.summary.skipped == 1 && full.summary.invalid == 1 &&
                     sizing.summary.no_room == 2 && full.dir[3].naxis1 == w2 && full.dir[3].naxis2 == h2 && full.dir[3].bytes == w2 * h2 &&
                     tight.summary.written == 1 && tight.summary.no_room == 1 &&
                     std::memcmp(tight.out.data(), full.out.data(), (size_t)tight.summary.units_bytes) == 0 &&
                     (w2 != w || std::memcmp(full.out.data() + RO_LEVEL_BLOCK, px.data(), px.size()) == 0);
            }
            std::printf("%5lld x %5lld %-7s width %4d  -> %4d x %4lld  %s\n", (long long)w, (long long)h, names[content], width, w2, (long long)h2,
                        ok ? "" : "MISMATCH");
            if (!ok) return 1;
        }
    if (call({}, 0, {}, 8, 0).summary.entries != 0) return 1;
    std::printf("ok\n");
    return 0;
}
