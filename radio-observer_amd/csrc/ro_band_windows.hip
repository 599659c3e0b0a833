// ro_band_windows.hip -- the band-only transform over a list of column windows (gfx950): at most 1024 columns of the
// fft-shifted row in up to eight runs, computed from the samples without the full-size transform and without a full row
// in HBM (ro_stft_band_windows_resident).  ro_band_windows.h has what differs from ro_band.h.
//
//   bandw_slab_kernel<M, A, FMT>  band_slab_kernel of ro_band.hip -- the same loads, levels, LDS image, xor tree, t1 / t2
//                                 layout by image column and slab partials -- whose gather reads the LDS cell of each
//                                 image column's bin from the host's table kcell instead of deriving it from first_col
//   bandw_finish_kernel           band_finish_kernel: adds a row's partials in slab order, takes the magnitude
//
// A file of its own, so that ro_band.hip and the consecutive call's code objects stay what they were: with the table
// read inside band_slab_kernel the FP64 twin of this change cost the existing call 0.4 - 1.5 % of its rate
// (profiles/band_windows.txt).  No atomics anywhere: two launches give the same bits, and a column has the bits
// band_slab_kernel gives it (the arithmetic of a column depends on its bin, M and A only).
#include "ro_band_windows.h"
#include "ro_kernels.h"

namespace ro {

namespace {

typedef float c2f __attribute__((ext_vector_type(2)));

__device__ __forceinline__ c2f band_cmul(c2f a, c2f w)
{
    return (c2f){a.x * w.x - a.y * w.y, a.y * w.x + a.x * w.y};
}

template <int FMT> struct BandSample;
template <> struct BandSample<RO_FMT_F32> {
    static constexpr int BYTES = 8;                     // rows start at any sample: 8-byte alignment is all there is
    static __device__ __forceinline__ c2f load(const char *row, int n)
    {
        const float2 x = reinterpret_cast<const float2 *>(row)[n];
        return (c2f){x.x, x.y};
    }
};
template <> struct BandSample<RO_FMT_I16> {
    static constexpr int BYTES = 4;
    static __device__ __forceinline__ c2f load(const char *row, int n)
    {
        const unsigned u = reinterpret_cast<const unsigned *>(row)[n];
        return (c2f){(float)(short)(u & 0xffffu), (float)(short)(u >> 16)};
    }
};

// one radix-4 level of span S of all A transforms, in place; T threads, A M / 4 butterflies
template <int M, int A, int S> __device__ __forceinline__ void band_radix4(c2f *cell, const float2 *__restrict__ tw, int tid)
{
    constexpr int Q = S / 4, T = A * M / 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int w = tid + T * i;                     // < A M / 4
        const int t = w % A, u = w / A;                // u < M / 4
        const int j = u % Q, base = (u / Q) * S + j;   // base + 3 Q < M
        c2f *p = cell + base * A + t;
        const c2f x0 = p[0], x1 = p[Q * A], x2 = p[2 * Q * A], x3 = p[3 * Q * A];
        const c2f s02 = x0 + x2, d02 = x0 - x2, s13 = x1 + x3, d13 = x1 - x3;
        const c2f md = (c2f){d13.y, -d13.x};           // -i (x1 - x3)
        c2f y0 = s02 + s13, y1 = d02 + md, y2 = s02 - s13, y3 = d02 - md;
        if constexpr (Q > 1) {
            constexpr int STEP = M / S;                // exp(-2 pi i q j / S) = tw[q j STEP], q j STEP < 3 M / 4
            const float2 w1 = tw[j * STEP], w2 = tw[2 * j * STEP], w3 = tw[3 * j * STEP];
            y1 = band_cmul(y1, (c2f){w1.x, w1.y});
            y2 = band_cmul(y2, (c2f){w2.x, w2.y});
            y3 = band_cmul(y3, (c2f){w3.x, w3.y});
        }
        p[0] = y0;
        p[Q * A] = y1;
        p[2 * Q * A] = y2;
        p[3 * Q * A] = y3;
    }
}

// the last level of M = 512: pairs of neighbouring cells, no twiddle
template <int M, int A> __device__ __forceinline__ void band_radix2_last(c2f *cell, int tid)
{
    constexpr int T = A * M / 16;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int w = tid + T * i;                     // < A M / 2
        const int t = w % A, u = w / A;
        c2f *p = cell + 2 * u * A + t;
        const c2f x0 = p[0], x1 = p[A];
        p[0] = x0 + x1;
        p[A] = x0 - x1;
    }
}

template <int M, int A, int S> __device__ __forceinline__ void band_levels(c2f *cell, const float2 *__restrict__ tw, int tid)
{
    if constexpr (S >= 4) {
        band_radix4<M, A, S>(cell, tw, tid);
        __syncthreads();
        band_levels<M, A, S / 4>(cell, tw, tid);
    } else if constexpr (S == 2) {
        band_radix2_last<M, A>(cell, tid);
        __syncthreads();
    }
}

template <int M, int A, int FMT>
__global__ __launch_bounds__(A * M / 16) void bandw_slab_kernel(BandWinArgs a)
{
    constexpr int T = A * M / 16;
    __shared__ __attribute__((aligned(16))) c2f cell[A * M];
    const int tid = threadIdx.x;
    const int slab = blockIdx.x, slabs = gridDim.x;
    const int64_t row = blockIdx.y;
    const int L = a.bins / M, a0 = slab * A;           // a0 + A <= L
    const char *src = reinterpret_cast<const char *>(a.iq) + (a.first_row + row) * (int64_t)a.hop * BandSample<FMT>::BYTES;

    // ---- samples: cell w = b A + t takes sample a0 + t + L b (< bins), all sixteen loads of a thread in flight
    {
        c2f x[16];
        float wn[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int w = tid + T * i;                 // < A M
            const int n = a0 + w % A + L * (w / A);
            x[i] = BandSample<FMT>::load(src, n);
            wn[i] = a.window[n];
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            x[i].y += a.gain;                          // src/FFTBackend.cpp:78-79: Q += gain, then the window
            cell[tid + T * i] = x[i] * wn[i];
        }
    }
    __syncthreads();

    // ---- the A transforms of M points
    band_levels<M, A, M>(cell, a.tw, tid);

    // ---- the slab's partial sum of every wanted column: A lanes per column, one per residue
    const int t = tid % A, g = tid / A;
    float2 *out = a.part + (row * slabs + slab) * (int64_t)a.cols;
    for (int j0 = 0; j0 < a.cols; j0 += T / A) {
        const int j = j0 + g;
        const bool live = j < a.cols;
        const int jj = live ? j : a.cols - 1;
        const c2f z = cell[a.kcell[jj] + t];           // kcell[jj] < A M, a multiple of A (the host's table)
        const float2 w1 = a.t1[jj * A + t];
        c2f p = band_cmul(z, (c2f){w1.x, w1.y});
#pragma unroll
        for (int m = A / 2; m >= 1; m >>= 1) {         // the same tree on every launch
            p.x += __shfl_xor(p.x, m, 64);
            p.y += __shfl_xor(p.y, m, 64);
        }
        if (live && t == 0) {
            const float2 w2 = a.t2[slab * a.cols + j];
            p = band_cmul(p, (c2f){w2.x, w2.y});
            out[j] = make_float2(p.x, p.y);
        }
    }
}

__global__ __launch_bounds__(256) void bandw_finish_kernel(const float2 *__restrict__ part, float *__restrict__ band_out,
                                                          int64_t band_stride, int cols, int slabs)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= cols) return;
    const int64_t row = blockIdx.y;
    const float2 *p = part + row * slabs * (int64_t)cols + j;
    float re = 0.0f, im = 0.0f;
    for (int s = 0; s < slabs; ++s) {                  // slab order, always
        const float2 v = p[(int64_t)s * cols];
        re += v.x;
        im += v.y;
    }
    band_out[row * band_stride + j] = __builtin_amdgcn_sqrtf(re * re + im * im);
}

template <int M, int A> hipError_t launch_wslab(int fmt, const BandWinArgs &a, int slabs, hipStream_t s)
{
    const dim3 grid((unsigned)slabs, (unsigned)a.rows), block(A * M / 16);
    if (fmt == RO_FMT_I16) hipLaunchKernelGGL((bandw_slab_kernel<M, A, RO_FMT_I16>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bandw_slab_kernel<M, A, RO_FMT_F32>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_band_windows(const BandPlan &p, int fmt, const BandWinArgs &a, hipStream_t s)
{
    if (a.rows <= 0) return hipSuccess;
    if (a.rows > 65535 || (fmt != RO_FMT_F32 && fmt != RO_FMT_I16)) return hipErrorInvalidValue;
    hipError_t e = p.m == 256   ? launch_wslab<256, 16>(fmt, a, p.slabs, s)
                   : p.m == 512 ? launch_wslab<512, 16>(fmt, a, p.slabs, s)
                                : launch_wslab<1024, 8>(fmt, a, p.slabs, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bandw_finish_kernel, dim3((unsigned)((a.cols + 255) / 256), (unsigned)a.rows), dim3(256), 0, s,
                       a.part, a.band_out, a.band_stride, a.cols, p.slabs);
    return hipGetLastError();
}

}  // namespace ro
