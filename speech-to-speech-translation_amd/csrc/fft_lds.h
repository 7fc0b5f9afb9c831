// Complex FFT of N points (256 ... 2048, powers of two) in LDS by one 256-thread workgroup: the Stockham passes that the
// Griffin-Lim kernels (infer.hip) and the feature-extraction kernels (features.hip) share.  Callers pack TWO real frames as
// the real and imaginary part of one transform and separate the spectra through the Hermitian symmetry.
#pragma once
#include "s2st_common.h"

namespace {

struct cplx { float x, y; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return cplx{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return cplx{a.x - b.x, a.y - b.y}; }

// LDS arrays are PADDED: logical element i lives at P(i) = i + (i >> 5).  The Stockham passes scatter their results with
// power-of-two strides (4, 16, 64 elements of 8 bytes) and read twiddles at strides of N / (4 Ns): without the pad 8 - 16
// lanes of a wave hit one bank (the first measurement of these kernels on MI355X: 390 us per 44.5 k-frame STFT, ~10 k cycles
// of a CU per frame pair against ~2 k of LDS traffic).
__device__ __forceinline__ int fpad(int i) { return i + (i >> 5); }
template <int N>
struct FftLds {
  static constexpr int SIZE = N + N / 32 + 1;
};

// in-place complex FFT of the padded LDS array buf (logical 0 .. N), 256 threads; tw (padded) logical j = exp(-2 pi i j / N);
// INV: conjugate transform (unscaled).  Stockham autosort passes of radix 8 while a factor 8 is left, then one radix-4 or
// radix-2 pass (2048 = 8 * 8 * 8 * 4: FOUR LDS round trips; the first form of this kernel ran five radix-4 passes and a
// radix-2 one with run-time strides).  Pass with Ns done: butterfly j (0 .. N / R) reads x_r = buf[j + r N / R] * w^(r k)
// with k = j mod Ns, w = exp(-+2 pi i / (R Ns)), and writes its R outputs to (j - k) R + k + s Ns.
template <bool INV>
__device__ __forceinline__ cplx mul_mi(cplx d) { return INV ? cplx{-d.y, d.x} : cplx{d.y, -d.x}; }  // d * (-+ i)
template <bool INV>
__device__ __forceinline__ cplx mul_w8(cplx d) {  // d * exp(-+ i pi / 4)
  constexpr float h = 0.70710678118654752440f;
  return INV ? cplx{h * (d.x - d.y), h * (d.x + d.y)} : cplx{h * (d.x + d.y), h * (d.y - d.x)};
}
template <bool INV>
__device__ __forceinline__ cplx mul_w83(cplx d) {  // d * exp(-+ 3 i pi / 4)
  constexpr float h = 0.70710678118654752440f;
  return INV ? cplx{-h * (d.x + d.y), h * (d.x - d.y)} : cplx{h * (d.y - d.x), -h * (d.x + d.y)};
}
template <int R, bool INV>
__device__ __forceinline__ void dft_small(cplx* v) {
  if constexpr (R == 2) {
    const cplx a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
  } else if constexpr (R == 4) {
    const cplx e0 = cadd(v[0], v[2]), e1 = csub(v[0], v[2]), e2 = cadd(v[1], v[3]), e3 = mul_mi<INV>(csub(v[1], v[3]));
    v[0] = cadd(e0, e2);
    v[1] = cadd(e1, e3);
    v[2] = csub(e0, e2);
    v[3] = csub(e1, e3);
  } else {
    // even outputs: 4-point transform of x_n + x_{n+4}; odd outputs: of (x_n - x_{n+4}) * w8^n
    cplx c[4] = {cadd(v[0], v[4]), cadd(v[1], v[5]), cadd(v[2], v[6]), cadd(v[3], v[7])};
    cplx d[4] = {csub(v[0], v[4]), mul_w8<INV>(csub(v[1], v[5])), mul_mi<INV>(csub(v[2], v[6])), mul_w83<INV>(csub(v[3], v[7]))};
    dft_small<4, INV>(c);
    dft_small<4, INV>(d);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q] = c[q];
      v[2 * q + 1] = d[q];
    }
  }
}
template <int N, int NS, int R, bool INV>
__device__ __forceinline__ void fft_pass(cplx* buf, const cplx* tw, int tid) {
  constexpr int NB = N / R, PER = (NB + 255) / 256, TS = N / (R * NS);
  cplx v[PER][R];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = tid + 256 * i;
    if (NB % 256 == 0 || j < NB) {
      const int k = j & (NS - 1);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        cplx x = buf[fpad(j + r * NB)];
        if (NS > 1 && r > 0) {
          cplx w = tw[fpad(r * k * TS)];
          if (INV) w.y = -w.y;
          x = cmul(x, w);
        }
        v[i][r] = x;
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = tid + 256 * i;
    if (NB % 256 == 0 || j < NB) {
      const int k = j & (NS - 1);
      dft_small<R, INV>(v[i]);
      const int j0 = (j - k) * R + k;
#pragma unroll
      for (int r = 0; r < R; ++r) buf[fpad(j0 + r * NS)] = v[i][r];
    }
  }
  __syncthreads();
}
template <int N, int NS, bool INV>
__device__ __forceinline__ void fft_passes(cplx* buf, const cplx* tw, int tid) {
  if constexpr (NS < N) {
    constexpr int R = N / NS >= 8 ? 8 : N / NS;
    fft_pass<N, NS, R, INV>(buf, tw, tid);
    fft_passes<N, NS * R, INV>(buf, tw, tid);
  }
}
template <int N, bool INV>
__device__ void fft_lds(cplx* buf, const cplx* tw, int tid) {
  fft_passes<N, 1, INV>(buf, tw, tid);
}

}  // namespace
