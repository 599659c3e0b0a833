// ro_cut_windows.hip -- up to RO_MAX_TILE_WINDOWS column windows of full rows side by side in one image: what several
// recorders keep of a row (every SnapshotRecorder / BolidRecorder cuts its own [leftBin, rightBin),
// src/WaterfallBackend.cpp:174-205, :368-374; WaterfallBackend holds a vector of them) in the layout of
// ro_stft_band_windows_resident -- window w at image floats [off_w, off_w + cols_w) of each row.  A plain streaming
// copy over rows that are already in HBM: every wanted float is read once and written once, one dword per lane, lanes of
// a wave on consecutive image columns -- consecutive addresses on both sides (except where a wave crosses from one
// window to the next) whatever first_col, off_w and the two strides are aligned to.
#include "ro_kernels.h"

namespace ro {

namespace {

constexpr int CUT_WAVES = 4;                    // waves of a workgroup, each on rows of its own
constexpr int CUT_STEPS = 4;                    // runs of 64 image columns per wave: a workgroup spans 256 columns ...
constexpr int CUT_PASSES = 2;                   // ... of CUT_WAVES * CUT_PASSES rows
constexpr int CUT_COLS = 64 * CUT_STEPS;
constexpr int CUT_ROWS = CUT_WAVES * CUT_PASSES;

// Workgroup b takes the `chunk`-th run of CUT_COLS image columns of the `group`-th run of CUT_ROWS rows, b = group *
// chunks + chunk.  The window list travels in the kernel arguments; every loop over it is unrolled, so its entries are
// read with constant indices (scalar loads, no table in memory, no scratch).  A lane looks its (up to) CUT_STEPS source
// columns up once and uses them for each of its rows; all loads of a lane are issued before its first store.
__global__ __launch_bounds__(64 * CUT_WAVES) void cut_windows_kernel(CutArgs a, unsigned chunks)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const unsigned group = blockIdx.x / chunks;
    const unsigned chunk = blockIdx.x - group * chunks;
    int src[CUT_STEPS];                          // column of the row behind image column j, -1: past the image
    int j0 = (int)(chunk * CUT_COLS) + lane;
#pragma unroll
    for (int k = 0; k < CUT_STEPS; ++k) {
        const int j = j0 + 64 * k;
        int shift = a.first[0];                  // source column - image column, of the window j lies in
#pragma unroll
        for (int w = 1; w < RO_MAX_TILE_WINDOWS; ++w)
            shift = j >= a.off[w] ? a.first[w] - a.off[w] : shift;      // (off[w] of the unused entries: INT32_MAX)
        src[k] = j < a.total ? j + shift : -1;
    }
    float v[CUT_PASSES][CUT_STEPS];
    const int64_t row0 = (int64_t)group * CUT_ROWS + wave;
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const int64_t row = row0 + CUT_WAVES * p;
        const float *in = a.rows_in + row * a.row_stride;
#pragma unroll
        for (int k = 0; k < CUT_STEPS; ++k)
            v[p][k] = (row < a.rows && src[k] >= 0) ? in[src[k]] : 0.0f;
    }
#pragma unroll
    for (int p = 0; p < CUT_PASSES; ++p) {
        const int64_t row = row0 + CUT_WAVES * p;
        float *out = a.image + row * a.image_stride + j0;
#pragma unroll
        for (int k = 0; k < CUT_STEPS; ++k)
            if (row < a.rows && src[k] >= 0) out[64 * k] = v[p][k];
    }
}

}  // namespace

hipError_t launch_cut_windows(const CutArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    if (a.count < 1 || a.count > RO_MAX_TILE_WINDOWS || a.total < 1 || a.off[0] != 0) return hipErrorInvalidValue;
    for (int w = 1; w < a.count; ++w)
        if (a.off[w] <= a.off[w - 1] || a.off[w] >= a.total) return hipErrorInvalidValue;
    const unsigned chunks = (unsigned)((a.total + CUT_COLS - 1) / CUT_COLS);
    // any number of rows: the grid is one-dimensional (2^31 - 1 workgroups at most), and a launch takes at most 2^30
    const int64_t groups_at_once = ((int64_t)1 << 30) / chunks;
    const int64_t groups = (a.rows + CUT_ROWS - 1) / CUT_ROWS;
    CutArgs all = a;
    for (int w = a.count; w < RO_MAX_TILE_WINDOWS; ++w) all.off[w] = INT32_MAX;      // never reached by an image column
    for (int64_t g = 0; g < groups; g += groups_at_once) {
        CutArgs part = all;
        part.rows_in = a.rows_in + g * CUT_ROWS * a.row_stride;
        part.image = a.image + g * CUT_ROWS * a.image_stride;
        part.rows = a.rows - g * CUT_ROWS;
        const int64_t n = groups - g < groups_at_once ? groups - g : groups_at_once;
        if (n < groups - g) part.rows = n * CUT_ROWS;
        hipLaunchKernelGGL(cut_windows_kernel, dim3((unsigned)(n * chunks)), dim3(64 * CUT_WAVES), 0, s, part, chunks);
    }
    return hipGetLastError();
}

}  // namespace ro
