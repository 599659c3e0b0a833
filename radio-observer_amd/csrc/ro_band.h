// ro_band.h -- launch interface of the band-only transform (ro_band.hip; internal, not part of the C ABI).
//
// Columns c in [first_col, first_col + cols) of the fft-shifted row, bin k(c) = (c + N/2) mod N, without the N-point
// transform: with M the smallest of {256, 512, 1024} >= cols, L = N / M and the windowed samples indexed n = a + L b,
//   Z_a[r] = sum_{b<M} y[a + L b] exp(-2 pi i b r / M)            L transforms of M points
//   X[k]   = sum_{a<L} exp(-2 pi i a k / N) Z_a[k mod M]          one L-term sum per wanted column
// A workgroup takes one row and a slab of A consecutive a, a0 = slab A: it leaves
//   part[row][slab][j] = exp(-2 pi i a0 k / N) sum_{t<A} exp(-2 pi i t k / N) Z_{a0+t}[k mod M],   k = k(first_col + j)
// and band_finish_kernel adds a row's L / A partials in slab order and takes the magnitude.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ro {

struct BandPlan {
    int m;        // points of the short transforms: 256, 512 or 1024
    int a;        // residues a per workgroup: 16, or 8 at m = 1024 (64 KiB of LDS, two workgroups per CU)
    int slabs;    // bins / (m a) workgroups per row
};
// false: no band kernel for this shape (bins a power of two 16384 ... 1048576, 1 <= cols <= 1024)
bool band_plan(int bins, int cols, BandPlan &p);

struct BandArgs {
    const void   *iq;          // sample 0 of the stream
    const float  *window;      // bins floats, natural order
    const float2 *tw;          // [m]: exp(-2 pi i j / m)
    const float2 *t1;          // [cols][a]: exp(-2 pi i t k(j) / bins)
    const float2 *t2;          // [slabs][cols]: exp(-2 pi i (slab a) k(j) / bins)
    float2       *part;        // scratch: [rows][slabs][cols]
    float        *band_out;    // [rows][band_stride]
    int64_t       first_row, rows, band_stride;
    int           hop, bins, first_col, cols;
    float         gain;
};
// rows <= 65535 per launch (the caller chunks)
hipError_t launch_band(const BandPlan &p, int fmt, const BandArgs &a, hipStream_t s);

}  // namespace ro
