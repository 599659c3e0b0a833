// ro_resize.hip -- resized previews on the device: fits2png's --width, which is Pillow's 8-bit Lanczos resize, over every
// level image a resize plan has a job for.  include/ro_stft.h states the rule; the taps are host arithmetic (ro_resize.cpp:
// they depend on the C library's sin in double), so what runs here is integer work only: an int32 sum of pixels times
// 22-bit taps, a shift and a clamp, the horizontal pass rounded to a byte before the vertical one reads it.  ro_resize.h has
// the plan blob and the checks: the blob is the caller's upload, so a job is checked against the buffers before anything of
// it is touched, and a tap's bounds are clamped into its image whatever the blob says.
//
// Two plain launches; no atomics, no floating point, no workgroup waits for another:
//   resize_h_kernel    a workgroup takes 64 output columns of 4 rows, a wave a row.  The input pixels the tile needs are one
//                      contiguous span of each row, from the first column's xmin to the last one's xmin + xmax; it is staged
//                      in LDS with 16-byte loads in pieces of 2048 columns -- the span of ONE output pixel can be longer than
//                      that (1641 taps at 70000 -> 256), so every lane adds up the taps of its pixel that fall into the piece
//                      and goes on with the next.  Tap x of the tile's columns is 64 neighbouring words.  The row goes to the
//                      intermediate image in handle scratch
//   resize_v_kernel    a workgroup takes 256 output columns of 4 rows, a wave a row and a lane four columns out of one 32-bit
//                      load: every tap reads a coalesced row of the intermediate image, and the tap is the wave's.  The same
//                      launch copies the images that keep their shape, 16 bytes a lane, and zeroes every image's pad up to
//                      its last 720-byte block
// All addressing is 64-bit; what is 32-bit are indices into ONE image, which has fewer than 2^31 pixels.
#include "ro_pack_plan.h"
#include "ro_resize.h"

namespace ro {

namespace {

constexpr int T = 256;
static_assert(T == 64 * RESIZE_HY && T == 64 * RESIZE_VY && RESIZE_HX == 64 && RESIZE_VX == 4 * 64 && RESIZE_PIECE % 16 == 0,
              "a wave per row; a lane per column, or per four");

// The job of work item p: the last of the jobs whose first item is at most p, or -1 (plan_entry over a field of the jobs)
template <bool H> __device__ __forceinline__ int64_t job_of(const ResizeJob *jobs, int64_t n, int64_t p)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((H ? jobs[mid].first_h : jobs[mid].first_v) <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// 16 bytes at byte `at` of a buffer of `bytes` (at: a multiple of 16 that is not negative); zeros past its end
__device__ __forceinline__ uint4 load16(const unsigned char *base, int64_t at, int64_t bytes)
{
    if (at + 16 <= bytes) return *reinterpret_cast<const uint4 *>(base + at);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (at + i < bytes) w[i >> 2] |= (unsigned)base[at + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(T) void resize_h_kernel(ResizeArgs a)
{
    if (!resize_head_ok(a.plan, a.plan_bytes)) return;
    const ResizePlanHead *head = reinterpret_cast<const ResizePlanHead *>(a.plan);
    const ResizeJob *jobs = reinterpret_cast<const ResizeJob *>(a.plan + sizeof(ResizePlanHead));
    const int64_t njobs = head->jobs, total = head->h_items < a.h_items ? head->h_items : a.h_items;
    const ResizeRooms rooms = {a.levels_bytes, a.out_levels_bytes, a.mid_bytes, a.plan_bytes};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ __attribute__((aligned(16))) unsigned char tile[RESIZE_HY][RESIZE_PIECE + 16];
#pragma unroll 1
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int64_t d = job_of<true>(jobs, njobs, item);
        if (d < 0) continue;
        const ResizeJob j = jobs[d];
        ResizeTable th = {}, tv = {};
        if (j.w == j.w_out || !resize_job_ok(a.plan, rooms, j, th, tv)) continue;
        const int64_t k = item - j.first_h;
        if (k < 0 || k >= resize_h_items(j.w_out, j.h)) continue;
        const int32_t tiles_x = (j.w_out + RESIZE_HX - 1) / RESIZE_HX;
        const int32_t y = (int32_t)(k / tiles_x) * RESIZE_HY + wave, xx = (int32_t)(k % tiles_x) * RESIZE_HX + lane;
        const bool row_live = y < j.h, live = row_live && xx < j.w_out;
        int32_t lo = 0, n = 0;
        if (xx < j.w_out) resize_bounds(th, xx, lo, n);
        // the span of the tile's columns: the same in every wave
        const int32_t span_lo = (int32_t)wave_min_u32(xx < j.w_out ? (unsigned)lo : 0x7fffffffu);
        const int32_t span_hi = (int32_t)wave_max_u32(xx < j.w_out ? (unsigned)(lo + n) : 0u);
        const int64_t row = j.src + (int64_t)(row_live ? y : 0) * j.w;       // byte of the levels where the row starts
        const int32_t *tap = th.taps + xx;
        int32_t sum = 1 << (RESIZE_BITS - 1);
#pragma unroll 1
        for (int32_t c0 = span_lo; c0 < span_hi; c0 += RESIZE_PIECE) {
            const int32_t cols = span_hi - c0 < RESIZE_PIECE ? span_hi - c0 : RESIZE_PIECE;
            const int64_t g = row + c0;
            const int shift = (int)(g & 15);
            wg_sync();                           // the piece before this one has been read
            if (row_live) {
                const int chunks = (shift + cols + 15) >> 4;
                for (int q = lane; q < chunks; q += 64)
                    *reinterpret_cast<uint4 *>(&tile[wave][16 * q]) = load16(a.levels, g - shift + 16 * (int64_t)q, a.levels_bytes);
            }
            wg_sync();
            if (live) {
                const int32_t x0 = c0 > lo ? c0 - lo : 0, x1 = n < c0 + cols - lo ? n : c0 + cols - lo;
                const unsigned char *px = &tile[wave][lo - c0 + shift];
                for (int32_t x = x0; x < x1; ++x) sum += (int32_t)px[x] * tap[(int64_t)x * j.w_out];
            }
        }
        if (live) {
            a.mid[j.mid + (int64_t)y * j.w_out + xx] = resize_clip(sum);
        }
    }
}

__global__ __launch_bounds__(T) void resize_v_kernel(ResizeArgs a)
{
    if (!resize_head_ok(a.plan, a.plan_bytes)) return;
    const ResizePlanHead *head = reinterpret_cast<const ResizePlanHead *>(a.plan);
    const ResizeJob *jobs = reinterpret_cast<const ResizeJob *>(a.plan + sizeof(ResizePlanHead));
    const int64_t njobs = head->jobs, total = head->v_items < a.v_items ? head->v_items : a.v_items;
    const ResizeRooms rooms = {a.levels_bytes, a.out_levels_bytes, a.mid_bytes, a.plan_bytes};
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll 1
    for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
        const int64_t d = job_of<false>(jobs, njobs, item);
        if (d < 0) continue;
        const ResizeJob j = jobs[d];
        ResizeTable th = {}, tv = {};
        if (!resize_job_ok(a.plan, rooms, j, th, tv)) continue;
        const bool vp = j.h != j.h_out;            // resized, both passes; else a copy
        const int64_t out_bytes = (int64_t)j.w_out * j.h_out;
        const int64_t work = vp ? resize_v_items(j.w_out, j.h_out) : resize_copy_items(out_bytes);
        const int64_t k = item - j.first_v;
        if (k < 0 || k > work) continue;
        unsigned char *dst = a.out_levels + j.dst;
        if (k == work) {                         // the pad: zeros up to the end of the image's last block
            const int64_t end = resize_up(out_bytes, RO_LEVEL_BLOCK);
            for (int64_t i = out_bytes + t; i < end; i += T) dst[i] = 0;
            continue;
        }
        if (!vp) {                               // the copy: both starts are multiples of 16 bytes
            const unsigned char *src = a.levels + j.src;
            const int64_t at0 = k * RESIZE_COPY, end = at0 + RESIZE_COPY < out_bytes ? at0 + RESIZE_COPY : out_bytes;
            for (int64_t at = at0 + 16 * t; at < end; at += 16 * T) {
                if (at + 16 <= end) *reinterpret_cast<uint4 *>(dst + at) = *reinterpret_cast<const uint4 *>(src + at);
                else
                    for (int64_t i = at; i < end; ++i) dst[i] = src[i];
            }
            continue;
        }
        const int32_t tiles_x = (j.w_out + RESIZE_VX - 1) / RESIZE_VX;
        const int32_t yy = (int32_t)(k / tiles_x) * RESIZE_VY + wave, c = (int32_t)(k % tiles_x) * RESIZE_VX + 4 * lane;
        if (yy >= j.h_out || c >= j.w_out) continue;
        const int left = j.w_out - c < 4 ? j.w_out - c : 4;   // columns of this lane
        int32_t lo, n;
        resize_bounds(tv, yy, lo, n);
        const unsigned char *in = a.mid + j.mid + (int64_t)lo * j.w_out + c;
        const int32_t *tap = tv.taps + yy;
        int32_t sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] = 1 << (RESIZE_BITS - 1);
        for (int32_t x = 0; x < n; ++x) {
            const int32_t kx = tap[(int64_t)x * j.h_out];
            const unsigned char *p = in + (int64_t)x * j.w_out;
            unsigned v = 0u;
            if (left == 4) __builtin_memcpy(&v, p, 4);
            else
                for (int i = 0; i < left; ++i) v |= (unsigned)p[i] << (8 * i);
#pragma unroll
            for (int i = 0; i < 4; ++i) sum[i] += (int32_t)((v >> (8 * i)) & 0xffu) * kx;
        }
        unsigned char *out = dst + (int64_t)yy * j.w_out + c;
        unsigned v = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) v |= (unsigned)resize_clip(sum[i]) << (8 * i);
        if (left == 4) __builtin_memcpy(out, &v, 4);
        else
            for (int i = 0; i < left; ++i) out[i] = (unsigned char)(v >> (8 * i));
    }
}

}  // namespace

hipError_t launch_levels_resize(const ResizeArgs &a, int cus, hipStream_t s)
{
    if (!a.plan || a.plan_bytes < (int64_t)sizeof(ResizePlanHead) || ((uintptr_t)a.plan & (RESIZE_ALIGN - 1)) != 0 || a.levels_bytes < 0 ||
        (a.levels_bytes > 0 && !a.levels) || ((uintptr_t)a.levels & (RESIZE_ALIGN - 1)) != 0 || a.out_levels_bytes < 0 ||
        (a.out_levels_bytes > 0 && !a.out_levels) || ((uintptr_t)a.out_levels & (RESIZE_ALIGN - 1)) != 0 || a.mid_bytes < 0 ||
        (a.mid_bytes > 0 && !a.mid) || ((uintptr_t)a.mid & (RESIZE_ALIGN - 1)) != 0 || a.h_items < 0 || a.v_items < 0)
        return hipErrorInvalidValue;
    // the work is the plan's, known on the host: no more workgroups than items, sixteen per CU at the most
    const unsigned most = 4 * copy_grid(cus);
    if (a.h_items > 0) hipLaunchKernelGGL(resize_h_kernel, dim3(png_grid_for(most, a.h_items, 1)), dim3(T), 0, s, a);
    if (a.v_items > 0) hipLaunchKernelGGL(resize_v_kernel, dim3(png_grid_for(most, a.v_items, 1)), dim3(T), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
