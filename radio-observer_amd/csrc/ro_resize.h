// ro_resize.h -- resized previews (ro_resize.hip, ro_resize.cpp): fits2png's --width, Pillow's 8-bit Lanczos resize to the
// byte.  include/ro_stft.h states the rule and the entry rules; this header has the plan blob -- what ro_resize_plan writes
// on the host and both the kernels and the host twin read -- the geometry of the work items, and the checks every reader of
// a plan makes before it touches a byte: a plan is the caller's upload, so nothing in it is trusted.
// The blob, every part at a multiple of 16 bytes:
//   ResizePlanHead                     64 bytes
//   ResizeJob[jobs]                    one per WRITTEN entry, in directory order; first_h / first_v never descend
//   the tap tables                     one per distinct (in, out) pair with in != out:
//       ResizeTableHead                16 bytes
//       int32 bounds[out][2]           xmin, xmax of every output pixel
//       int32 taps[ksize][out]         tap x of output pixel xx at [x * out + xx]: lanes on neighbouring pixels read
//                                      neighbouring words; zero at and behind xmax
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ro_stft.h"
#include "ro_png.h"

namespace ro {

constexpr int64_t RESIZE_MAGIC = 0x31455a4953455252ll;   // "RRESIZE1"
constexpr int RESIZE_BITS = 22;                  // of a fixed-point tap: 32 - 8 - 2, what an int32 sum of 8-bit pixels leaves
constexpr int RESIZE_ALIGN = 16;

// the horizontal pass: a workgroup takes RESIZE_HX output columns of RESIZE_HY rows, a wave a row, a lane a column
constexpr int RESIZE_HX = 64, RESIZE_HY = 4;
// ... and stages the input in pieces of RESIZE_PIECE columns per row (16 more bytes for where the row starts in its word)
constexpr int RESIZE_PIECE = 2048;
// the vertical pass: RESIZE_VX output columns (four to a lane) of RESIZE_VY rows, a wave a row
constexpr int RESIZE_VX = 256, RESIZE_VY = 4;
// the copy of an image that keeps its shape: bytes of a work item
constexpr int RESIZE_COPY = 16384;

struct ResizePlanHead {
    int64_t magic, jobs, h_items, v_items, mid_bytes, plan_bytes, reserved[2];
};

struct ResizeJob {
    int64_t src;                   // byte of the levels that is pixel 0
    int64_t dst;                   // ... of the out levels, a multiple of RO_LEVEL_BLOCK
    int64_t mid;                   // ... of the intermediate image, w_out x h bytes, of a job that is resized
    int64_t first_h;               // work item of the first launch where this job's start: the horizontal pass
    int64_t first_v;               // ... of the second: the vertical pass or the copy, and one item that zeroes the pad
    int64_t table_h;               // byte of the blob where the table of (w, w_out) starts; 0: the job is a copy
    int64_t table_v;               // ... of (h, h_out)
    int32_t w, h, w_out, h_out;    // a job runs BOTH passes or is a copy: where width < w, h_out = (int64)(h width / w) is
    int64_t reserved;              // below h too, and otherwise the image keeps its shape; resize_job_ok refuses the rest
};

struct ResizeTableHead {
    int32_t in, out, ksize, reserved;
};

static_assert(sizeof(ResizePlanHead) == 64 && sizeof(ResizeJob) == 80 && sizeof(ResizeTableHead) == 16, "the blob is these");

__host__ __device__ inline int64_t resize_up(int64_t x, int64_t to) { return (x + to - 1) / to * to; }
__host__ __device__ inline int64_t resize_table_bytes(int64_t out, int64_t ksize)
{
    return resize_up((int64_t)sizeof(ResizeTableHead) + 8 * out + 4 * out * ksize, RESIZE_ALIGN);
}
__host__ __device__ inline int64_t resize_h_items(int64_t w_out, int64_t h)
{
    return ((w_out + RESIZE_HX - 1) / RESIZE_HX) * ((h + RESIZE_HY - 1) / RESIZE_HY);
}
// the second launch's items of a resized job but the pad's
__host__ __device__ inline int64_t resize_v_items(int64_t w_out, int64_t h_out)
{
    return ((w_out + RESIZE_VX - 1) / RESIZE_VX) * ((h_out + RESIZE_VY - 1) / RESIZE_VY);
}
__host__ __device__ inline int64_t resize_copy_items(int64_t bytes) { return (bytes + RESIZE_COPY - 1) / RESIZE_COPY; }

// a table as a reader sees it, or null pointers where the blob does not hold all of it or it is not of (in, out)
struct ResizeTable {
    const int32_t *bounds, *taps;
    int32_t in, out, ksize;
};
__host__ __device__ inline bool resize_table(const char *plan, int64_t plan_bytes, int64_t at, int32_t in, int32_t out, ResizeTable &t)
{
    if (at < (int64_t)sizeof(ResizePlanHead) || at % RESIZE_ALIGN != 0 || at > plan_bytes - (int64_t)sizeof(ResizeTableHead)) return false;
    const ResizeTableHead *head = reinterpret_cast<const ResizeTableHead *>(plan + at);
    if (head->in != in || head->out != out || head->ksize < 1 || in < 1 || out < 1) return false;
    if (resize_table_bytes(out, head->ksize) > plan_bytes - at) return false;
    t.bounds = reinterpret_cast<const int32_t *>(plan + at + sizeof(ResizeTableHead));
    t.taps = t.bounds + 2 * (int64_t)out;
    t.in = in;
    t.out = out;
    t.ksize = head->ksize;
    return true;
}
// the taps of output pixel xx: input pixels [lo, lo + n), inside [0, in) whatever the blob says
__host__ __device__ inline void resize_bounds(const ResizeTable &t, int32_t xx, int32_t &lo, int32_t &n)
{
    const int32_t a = t.bounds[2 * (int64_t)xx], b = t.bounds[2 * (int64_t)xx + 1];
    lo = a < 0 ? 0 : (a > t.in ? t.in : a);
    const int32_t most = t.in - lo < t.ksize ? t.in - lo : t.ksize;
    n = b < 0 ? 0 : (b > most ? most : b);
}

// what the readers of a blob ask of its head: the blob is all there and the jobs lie in it
__host__ __device__ inline bool resize_head_ok(const char *plan, int64_t plan_bytes)
{
    if (!plan || plan_bytes < (int64_t)sizeof(ResizePlanHead)) return false;
    const ResizePlanHead *head = reinterpret_cast<const ResizePlanHead *>(plan);
    return head->magic == RESIZE_MAGIC && head->plan_bytes == plan_bytes && head->jobs >= 0 && head->mid_bytes >= 0 &&
           head->jobs <= (plan_bytes - (int64_t)sizeof(ResizePlanHead)) / (int64_t)sizeof(ResizeJob);
}

// a job checked against the buffers of the call before anything of it is touched; th / tv: its tables, where a pass runs
struct ResizeRooms {
    int64_t levels_bytes, out_levels_bytes, mid_bytes, plan_bytes;
};
__host__ __device__ inline bool resize_job_ok(const char *plan, const ResizeRooms &r, const ResizeJob &j, ResizeTable &th, ResizeTable &tv)
{
    int64_t raw, blocks, idat;
    // (what png_shape passes has fewer than 2^31 pixels)
    if (!png_shape(j.w, j.h, &raw, &blocks, &idat) || !png_shape(j.w_out, j.h_out, &raw, &blocks, &idat)) return false;
    if (!png_shape(j.w_out, j.h, &raw, &blocks, &idat)) return false;
    const int64_t in_bytes = (int64_t)j.w * j.h, out_bytes = (int64_t)j.w_out * j.h_out;
    if (j.src < 0 || j.src % RO_LEVEL_BLOCK != 0 || j.src > r.levels_bytes || in_bytes > r.levels_bytes - j.src) return false;
    if (j.dst < 0 || j.dst % RO_LEVEL_BLOCK != 0 || j.dst > r.out_levels_bytes ||
        resize_up(out_bytes, RO_LEVEL_BLOCK) > r.out_levels_bytes - j.dst)
        return false;
    const bool hp = j.w != j.w_out, vp = j.h != j.h_out;
    if (hp != vp) return false;                  // (one pass alone: not a job of ro_resize_plan)
    if (hp && vp && (j.mid < 0 || j.mid % RESIZE_ALIGN != 0 || j.mid > r.mid_bytes || (int64_t)j.w_out * j.h > r.mid_bytes - j.mid)) return false;
    if (hp && !resize_table(plan, r.plan_bytes, j.table_h, j.w, j.w_out, th)) return false;
    if (vp && !resize_table(plan, r.plan_bytes, j.table_v, j.h, j.h_out, tv)) return false;
    return j.first_h >= 0 && j.first_v >= 0;
}

// one output pixel from its taps: Pillow's clip8 of an int32 sum that starts at a half
__host__ __device__ inline unsigned char resize_clip(int32_t sum)
{
    const int32_t v = sum >> RESIZE_BITS;        // arithmetic
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct ResizeArgs {
    const char          *plan;                   // device: the caller's upload of the blob
    int64_t              plan_bytes;
    const unsigned char *levels;
    int64_t              levels_bytes;
    unsigned char       *out_levels;
    int64_t              out_levels_bytes;
    unsigned char       *mid;                    // scratch
    int64_t              mid_bytes;
    int64_t              h_items, v_items;       // the host's: they size the grids, the kernels go by the blob's
};

// the two passes on `s`: two launches; cus: the device's compute units
hipError_t launch_levels_resize(const ResizeArgs &a, int cus, hipStream_t s);

}  // namespace ro
