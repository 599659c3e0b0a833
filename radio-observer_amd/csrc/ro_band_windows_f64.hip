// ro_band_windows_f64.hip -- the band-only transform over a list of column windows in the reference's arithmetic (gfx950):
// at most 1024 columns of the fft-shifted row in up to eight runs, on RO_PRECISION_F64 handles of 131072 ... 1048576 bins
// (ro_stft_band_windows_resident).  ro_band_windows.h has what differs from ro_band_f64.h.
//
//   band64w_slab_kernel<M, A, FMT>  band64_slab_kernel of ro_band_f64.hip -- the same loads, levels, swizzled LDS image
//                                   (band64w_phys = band64_phys), xor tree, t1 / t2 layout by image column and slab
//                                   partials -- whose gather reads the logical LDS cell of each image column's bin from
//                                   the host's table kcell instead of deriving it from first_col
//   band64w_finish_kernel           band64_finish_kernel: slab order, double square root, narrowed once
//
// A file of its own, so that ro_band_f64.hip and the consecutive call's code objects stay what they were: with the table
// read inside band64_slab_kernel the existing call lost 0.4 - 1.5 % of its rate at A = 4 (profiles/band_windows.txt).
// tools/band/emu_band_windows.py walks the gather against numpy's FFT and counts its LDS cycles.
#include "ro_band_windows.h"
#include "ro_kernels.h"

#ifndef RO_FMT_F64
#define RO_FMT_F64 RO_IQ_F64
#endif

namespace ro {

namespace {

typedef double c2d __attribute__((ext_vector_type(2)));

constexpr int B64_T = 512;          // threads per workgroup
constexpr int B64_CELLS = 4096;     // double2 cells per workgroup: A M

__device__ __forceinline__ c2d band64_cmul(c2d a, c2d w)
{
    return (c2d){a.x * w.x - a.y * w.y, a.y * w.x + a.x * w.y};
}

template <int FMT> struct Band64Sample;
template <> struct Band64Sample<RO_FMT_F32> {
    static constexpr int BYTES = 8;                     // rows start at any sample: 8-byte alignment is all there is
    static __device__ __forceinline__ c2d load(const char *row, int n)
    {
        const float2 x = reinterpret_cast<const float2 *>(row)[n];
        return (c2d){(double)x.x, (double)x.y};
    }
};
template <> struct Band64Sample<RO_FMT_I16> {
    static constexpr int BYTES = 4;
    static __device__ __forceinline__ c2d load(const char *row, int n)
    {
        const unsigned u = reinterpret_cast<const unsigned *>(row)[n];
        return (c2d){(double)(short)(u & 0xffffu), (double)(short)(u >> 16)};
    }
};
template <> struct Band64Sample<RO_FMT_F64> {           // struct Complex {double real, imag;} (src/Backend.h:26-29)
    static constexpr int BYTES = 16;
    static __device__ __forceinline__ c2d load(const char *row, int n)
    {
        const double2 x = reinterpret_cast<const double2 *>(row)[n];
        return (c2d){x.x, x.y};
    }
};

// physical cell of logical cell c = b A + t (a permutation of [0, 4096): only bits of c below b's bit 2 change, by bits
// from b's bit 2 up)
template <int A> __device__ __forceinline__ int band64w_phys(int c)
{
    if constexpr (A == 16) {
        return c;
    } else if constexpr (A == 8) {
        const int b = c >> 3;
        return c ^ ((((b >> 2) ^ (b >> 7)) & 1) << 3);
    } else {
        const int b = c >> 2;
        const int x = (((b >> 2) ^ (b >> 3) ^ (b >> 8)) & 1) | ((((b >> 2) ^ (b >> 9)) & 1) << 1);
        return c ^ (x << 2);
    }
}

// one radix-4 level of span S of all A transforms, in place; 1024 butterflies, two per thread
template <int M, int A, int S> __device__ __forceinline__ void band64_radix4(c2d *cell, const double2 *__restrict__ tw, int tid)
{
    constexpr int Q = S / 4;
#pragma unroll
    for (int i = 0; i < B64_CELLS / 4 / B64_T; ++i) {
        const int w = tid + B64_T * i;                 // < 1024 = A M / 4
        const int t = w % A, u = w / A;                // u < M / 4
        const int j = u % Q, base = (u / Q) * S + j;   // base + 3 Q < M
        const int c = base * A + t;
        const int i0 = band64w_phys<A>(c), i1 = band64w_phys<A>(c + Q * A), i2 = band64w_phys<A>(c + 2 * Q * A),
                  i3 = band64w_phys<A>(c + 3 * Q * A);
        const c2d x0 = cell[i0], x1 = cell[i1], x2 = cell[i2], x3 = cell[i3];
        const c2d s02 = x0 + x2, d02 = x0 - x2, s13 = x1 + x3, d13 = x1 - x3;
        const c2d md = (c2d){d13.y, -d13.x};           // -i (x1 - x3)
        c2d y0 = s02 + s13, y1 = d02 + md, y2 = s02 - s13, y3 = d02 - md;
        if constexpr (Q > 1) {
            constexpr int STEP = M / S;                // exp(-2 pi i q j / S) = tw[q j STEP], q j STEP < 3 M / 4
            const double2 w1 = tw[j * STEP], w2 = tw[2 * j * STEP], w3 = tw[3 * j * STEP];
            y1 = band64_cmul(y1, (c2d){w1.x, w1.y});
            y2 = band64_cmul(y2, (c2d){w2.x, w2.y});
            y3 = band64_cmul(y3, (c2d){w3.x, w3.y});
        }
        cell[i0] = y0;
        cell[i1] = y1;
        cell[i2] = y2;
        cell[i3] = y3;
    }
}

// the last level of M = 512: pairs of neighbouring cells, no twiddle; 2048 butterflies, four per thread
template <int M, int A> __device__ __forceinline__ void band64_radix2_last(c2d *cell, int tid)
{
#pragma unroll
    for (int i = 0; i < B64_CELLS / 2 / B64_T; ++i) {
        const int w = tid + B64_T * i;                 // < 2048 = A M / 2
        const int t = w % A, u = w / A;
        const int c = 2 * u * A + t;
        const int i0 = band64w_phys<A>(c), i1 = band64w_phys<A>(c + A);
        const c2d x0 = cell[i0], x1 = cell[i1];
        cell[i0] = x0 + x1;
        cell[i1] = x0 - x1;
    }
}

template <int M, int A, int S> __device__ __forceinline__ void band64_levels(c2d *cell, const double2 *__restrict__ tw, int tid)
{
    if constexpr (S >= 4) {
        band64_radix4<M, A, S>(cell, tw, tid);
        __syncthreads();
        band64_levels<M, A, S / 4>(cell, tw, tid);
    } else if constexpr (S == 2) {
        band64_radix2_last<M, A>(cell, tid);
        __syncthreads();
    }
}

template <int M, int A, int FMT>
__global__ __launch_bounds__(B64_T) void band64w_slab_kernel(Band64WinArgs a)
{
    static_assert(M * A == B64_CELLS, "64 KiB of double2 cells");
    constexpr int PER = B64_CELLS / B64_T;             // 8 cells per thread
    __shared__ __attribute__((aligned(16))) c2d cell[B64_CELLS];
    const int tid = threadIdx.x;
    // (slab is blockIdx.x: the slabs that share a row's 128-byte lines -- at A = 4 a slab uses 16 bytes (int16), 32
    // (float32) or 64 (double) of each -- are dispatched together)
    const int slab = blockIdx.x, slabs = gridDim.x;
    const int64_t row = blockIdx.y;
    const int L = a.bins / M, a0 = slab * A;           // a0 + A <= L
    const char *src = reinterpret_cast<const char *>(a.iq) + (a.first_row + row) * (int64_t)a.hop * Band64Sample<FMT>::BYTES;

    // ---- samples: logical cell w = b A + t takes sample a0 + t + L b (< bins), all eight loads of a thread in flight
    {
        c2d x[PER];
        float wn[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int w = tid + B64_T * i;             // < 4096
            const int n = a0 + w % A + L * (w / A);
            x[i] = Band64Sample<FMT>::load(src, n);
            wn[i] = a.window[n];
        }
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const double wd = (double)wn[i];
            x[i].y += a.gain;                          // src/FFTBackend.cpp:78-79: Q += gain, then the window (:229-232)
            cell[band64w_phys<A>(tid + B64_T * i)] = (c2d){x[i].x * wd, x[i].y * wd};
        }
    }
    __syncthreads();

    // ---- the A transforms of M points
    band64_levels<M, A, M>(cell, a.tw, tid);

    // ---- the slab's partial sum of every wanted column: A lanes per column, one per residue
    const int t = tid % A, g = tid / A;
    double2 *out = a.part + (row * slabs + slab) * (int64_t)a.cols;
    for (int j0 = 0; j0 < a.cols; j0 += B64_T / A) {
        const int j = j0 + g;
        const bool live = j < a.cols;
        const int jj = live ? j : a.cols - 1;
        const c2d z = cell[band64w_phys<A>(a.kcell[jj] + t)];      // kcell[jj]: logical cell, < 4096, a multiple of A
        const double2 w1 = a.t1[jj * A + t];
        c2d p = band64_cmul(z, (c2d){w1.x, w1.y});
#pragma unroll
        for (int m = A / 2; m >= 1; m >>= 1) {         // the same tree on every launch (both dwords of each double)
            p.x += __shfl_xor(p.x, m, 64);
            p.y += __shfl_xor(p.y, m, 64);
        }
        if (live && t == 0) {
            const double2 w2 = a.t2[(int64_t)slab * a.cols + j];
            p = band64_cmul(p, (c2d){w2.x, w2.y});
            out[j] = make_double2(p.x, p.y);
        }
    }
}

__global__ __launch_bounds__(256) void band64w_finish_kernel(const double2 *__restrict__ part, float *__restrict__ band_out,
                                                            int64_t band_stride, int cols, int slabs)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= cols) return;
    const int64_t row = blockIdx.y;
    const double2 *p = part + row * slabs * (int64_t)cols + j;
    double re = 0.0, im = 0.0;
    for (int s = 0; s < slabs; ++s) {                  // slab order, always
        const double2 v = p[(int64_t)s * cols];
        re += v.x;
        im += v.y;
    }
    band_out[row * band_stride + j] = (float)sqrt(re * re + im * im);
}

template <int M, int A> hipError_t launch_wslab64(int fmt, const Band64WinArgs &a, int slabs, hipStream_t s)
{
    const dim3 grid((unsigned)slabs, (unsigned)a.rows), block(B64_T);
    if (fmt == RO_FMT_I16) hipLaunchKernelGGL((band64w_slab_kernel<M, A, RO_FMT_I16>), grid, block, 0, s, a);
    else if (fmt == RO_FMT_F64) hipLaunchKernelGGL((band64w_slab_kernel<M, A, RO_FMT_F64>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((band64w_slab_kernel<M, A, RO_FMT_F32>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_band64_windows(const Band64Plan &p, int fmt, const Band64WinArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    if (a.rows > 65535 || (fmt != RO_FMT_F32 && fmt != RO_FMT_I16 && fmt != RO_FMT_F64)) return hipErrorInvalidValue;
    hipError_t e = p.m == 256   ? launch_wslab64<256, 16>(fmt, a, p.slabs, s)
                   : p.m == 512 ? launch_wslab64<512, 8>(fmt, a, p.slabs, s)
                                : launch_wslab64<1024, 4>(fmt, a, p.slabs, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(band64w_finish_kernel, dim3((unsigned)((a.cols + 255) / 256), (unsigned)a.rows), dim3(256), 0, s,
                       a.part, a.band_out, a.band_stride, a.cols, p.slabs);
    return hipGetLastError();
}

}  // namespace ro
