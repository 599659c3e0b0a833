// ro_band_windows.h -- launch interface of the band-only transform over a list of column windows (ro_band_windows.hip,
// ro_band_windows_f64.hip; internal, not part of the C ABI).  The decomposition, the plans and the tables are ro_band.h's
// and ro_band_f64.h's:
//   X[k] = sum_{a<L} exp(-2 pi i a k / N) Z_a[k mod M]
// Nothing there asks the wanted k to be consecutive or their residues k mod M to be distinct (two columns of one residue
// read the same Z_a cell, each with its own twiddles).  Image column j shows bin k(j); which bins those are is the host's
// choice, told to the kernels by three tables indexed by image column: t1, t2 as before and
//   kcell[j] = band_cell(m, k(j) mod m) a      the LDS cell (FP64: the logical cell) of residue t = 0 of that bin
// -- the cell rather than the bin, so that the digit reversal is done once on the host and not in the gather loop.
#pragma once

#include "ro_band.h"
#include "ro_band_f64.h"

namespace ro {

// cell index b of result r of an m-point transform after the in-place levels (radix 4 while the span allows, then 2):
// the level of span S sends result digit r mod R to sub-block (r mod R) S / R (band_pos of ro_band.hip)
inline int band_cell(int m, int r)
{
    int pos = 0;
    for (int s = m; s > 1;) {
        const int radix = s >= 4 ? 4 : 2;
        pos += (r % radix) * (s / radix);
        r /= radix;
        s /= radix;
    }
    return pos;
}

struct BandWinArgs {
    const void    *iq;          // sample 0 of the stream
    const float   *window;      // bins floats, natural order
    const float2  *tw;          // [m]: exp(-2 pi i j / m)
    const float2  *t1;          // [cols][a]: exp(-2 pi i t k(j) / bins)
    const float2  *t2;          // [slabs][cols]: exp(-2 pi i (slab a) k(j) / bins)
    const int32_t *kcell;       // [cols]: < a m, a multiple of a
    float2        *part;        // scratch: [rows][slabs][cols]
    float         *band_out;    // [rows][band_stride]
    int64_t        first_row, rows, band_stride;
    int            hop, bins, cols;
    float          gain;
};
// the plan is band_plan(bins, cols) with cols the windows' total; rows <= 65535 per launch (the caller chunks)
hipError_t launch_band_windows(const BandPlan &p, int fmt, const BandWinArgs &a, hipStream_t s);

struct Band64WinArgs {
    const void    *iq;          // sample 0 of the stream (RO_FMT_F32, RO_FMT_I16 or RO_FMT_F64)
    const float   *window;
    const double2 *tw;
    const double2 *t1;
    const double2 *t2;
    const int32_t *kcell;       // [cols]: logical cell, < 4096, a multiple of a
    double2       *part;
    float         *band_out;
    int64_t        first_row, rows, band_stride;
    int            hop, bins, cols;
    double         gain;
};
// the plan is band64_plan(bins, cols) with cols the windows' total
hipError_t launch_band64_windows(const Band64Plan &p, int fmt, const Band64WinArgs &a, hipStream_t s);

}  // namespace ro
