// ro_scan_sets.hip -- the band scan of BolidRecorder::update (src/BolidRecorder.cpp:121-132, :313-347) for the EXTRA band
// sets of a handle (ro_stft_set_extra_bands): several detectors on one waterfall, each with its own noise band, detect
// band and averaging range (src/WaterfallBackend.cpp:534-536 calls every recorder for every row; src/BolidRecorder.cpp:
// 84-104 derives each one's bands).  One wavefront per (row, set) pair over rows that are already in HBM -- just written
// by the transform, so a pair meets its row in L2.  The primary set keeps its own path (scan_kernel, or the fused
// epilogue of the N = 32768 plan); the arithmetic is the very same device functions (ro_device_util.h), so a set equal
// to the primary gives the primary's bits.
#include "ro_device_util.h"

namespace ro {

namespace {

constexpr int SCAN_WAVES = 4;         // (row, set) pairs per workgroup, like scan_kernel's rows per workgroup

// Pair i = blockIdx.x * SCAN_WAVES + wave is set i % count of row i / count: the sets of a row sit in neighbouring waves.
// The bands travel in the kernel arguments and are picked with a wave-uniform index (scalar loads, no table in memory).
// E as in scan_kernel: bands up to 64 E columns are loaded once into registers; the cached / re-reading form of
// scan_noise is chosen per set by its noise width, which is uniform over the wave.  The 256-word histogram is the
// wave's own and is only ever touched by that wave (no workgroup barrier anywhere, so the early return is safe).
template <int E> __global__ __launch_bounds__(64 * SCAN_WAVES) void scan_sets_kernel(ScanSetsArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t i = (int64_t)blockIdx.x * SCAN_WAVES + wave;
    if (i >= a.rows * a.count) return;
    const int64_t row = i / a.count;
    const int set = (int)(i - row * a.count);
    const ro_bands_t b = a.sets[set];
    const GlobalRow src{a.rows_in + row * a.row_stride};
    __shared__ __attribute__((aligned(16))) unsigned hist[SCAN_WAVES][256];
    unsigned *h = hist[wave];
    const bool cached = b.noise_width <= 64 * E;
    const float noise = cached ? scan_noise<E>(src, b.low_noise, b.noise_width, h, lane)
                               : scan_noise<0>(src, b.low_noise, b.noise_width, h, lane);
    const int peak = scan_peak<E>(src, b.low_detect, b.detect_width, lane);
    const float avg = scan_average(src, b.low_detect + peak - b.avg_bins / 2, b.avg_bins, a.bins, lane);
    if (lane == 0) {
        ro_scan_record_t rec;
        rec.noise = noise;
        rec.peak = peak;
        rec.average = avg;
        a.extra[i] = rec;               // = extra[row * count + set]
    }
}

}  // namespace

hipError_t launch_scan_sets(const ScanSetsArgs &a, hipStream_t s)
{
    if (a.rows <= 0 || a.count <= 0) return hipSuccess;
    if (a.count > RO_MAX_EXTRA_BANDS) return hipErrorInvalidValue;
    const int64_t pairs = a.rows * a.count;
    const unsigned grid = (unsigned)((pairs + SCAN_WAVES - 1) / SCAN_WAVES);
    int widest = 0;
    for (int i = 0; i < a.count; ++i) {
        widest = a.sets[i].noise_width > widest ? a.sets[i].noise_width : widest;
        widest = a.sets[i].detect_width > widest ? a.sets[i].detect_width : widest;
    }
    // the same three steps as launch_scan
    if (widest <= 64 * SCAN_E) hipLaunchKernelGGL(scan_sets_kernel<SCAN_E>, dim3(grid), dim3(64 * SCAN_WAVES), 0, s, a);
    else if (widest <= 64 * 64) hipLaunchKernelGGL(scan_sets_kernel<64>, dim3(grid), dim3(64 * SCAN_WAVES), 0, s, a);
    else hipLaunchKernelGGL(scan_sets_kernel<128>, dim3(grid), dim3(64 * SCAN_WAVES), 0, s, a);
    return hipGetLastError();
}

}  // namespace ro
