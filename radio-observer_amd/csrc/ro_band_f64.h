// ro_band_f64.h -- launch interface of the band-only transform in the reference's arithmetic (ro_band_f64.hip; internal,
// not part of the C ABI).  The decomposition is ro_band.h's, every value a double:
//   Z_a[r] = sum_{b<M} y[a + L b] exp(-2 pi i b r / M)            L transforms of M points
//   X[k]   = sum_{a<L} exp(-2 pi i a k / N) Z_a[k mod M]          one L-term sum per wanted column
// with M the smallest of {256, 512, 1024} >= cols and L = N / M.  A workgroup takes one row and a slab of A = 4096 / M
// consecutive a (64 KiB of double2 cells) and leaves the slab's twiddled partial sum of every wanted column;
// band64_finish_kernel adds a row's N / 4096 partials in slab order, takes the double square root and narrows once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ro {

struct Band64Plan {
    int m;        // points of the short transforms: 256, 512 or 1024
    int a;        // residues a per workgroup: 4096 / m = 16, 8 or 4
    int slabs;    // bins / 4096 workgroups per row
};
// false: no FP64 band kernel for this shape (bins a power of two 131072 ... 1048576, 1 <= cols <= 1024; up to 65536
// bins an FP64 handle's full row never leaves the CU's registers, ro_f64reg.hip)
bool band64_plan(int bins, int cols, Band64Plan &p);

struct Band64Args {
    const void    *iq;          // sample 0 of the stream (RO_FMT_F32, RO_FMT_I16 or RO_FMT_F64)
    const float   *window;      // bins floats, natural order (the reference's table is float: src/FFTBackend.cpp:229-232)
    const double2 *tw;          // [m]: exp(-2 pi i j / m)
    const double2 *t1;          // [cols][a]: exp(-2 pi i t k(j) / bins)
    const double2 *t2;          // [slabs][cols]: exp(-2 pi i (slab a) k(j) / bins)
    double2       *part;        // scratch: [rows][slabs][cols]
    float         *band_out;    // [rows][band_stride]
    int64_t        first_row, rows, band_stride;
    int            hop, bins, first_col, cols;
    double         gain;
};
// rows <= 65535 per launch (the caller chunks)
hipError_t launch_band64(const Band64Plan &p, int fmt, const Band64Args &a, hipStream_t s);

}  // namespace ro
