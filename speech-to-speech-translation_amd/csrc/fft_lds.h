// Complex FFT of N points in LDS by one 256-thread workgroup: the Stockham passes that the Griffin-Lim kernels (infer.hip) and
// the feature-extraction kernels (features.hip) share.  Callers pack TWO real frames as the real and imaginary part of one
// transform and separate the spectra through the Hermitian symmetry.
// Sizes: the powers of two 256 ... 2048 (radix 8 / 4 / 2) and the mixed sizes 240, 400 and 1200 = 2^4 * 3 * 5^2 (radix 8 / 6 /
// 5 / 2; 1200 is the n_fft that stage 3 of the recipe writes into config.yaml).  THE LISTS BELOW are the only place that
// names the sizes: the dispatch switches of infer.hip / features.hip and the s2st_*_supported queries expand from them.
#pragma once
#include "s2st_common.h"

#define S2ST_FFT_POW2_SIZES(X) X(256) X(512) X(1024) X(2048)
#define S2ST_FFT_MIXED_SIZES(X) X(240) X(400) X(1200)

namespace {

struct cplx { float x, y; };
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return cplx{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return cplx{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return cplx{a.x - b.x, a.y - b.y}; }

// LDS arrays are PADDED: logical element i lives at P(i) = i + (i >> 5).  The Stockham passes scatter their results with
// power-of-two strides (4, 16, 64 elements of 8 bytes) and read twiddles at strides of N / (4 Ns): without the pad 8 - 16
// lanes of a wave hit one bank (the first measurement of these kernels on MI355X: 390 us per 44.5 k-frame STFT, ~10 k cycles
// of a CU per frame pair against ~2 k of LDS traffic).
// The mixed sizes keep this pad.  Their data reads are contiguous and their scatter strides 5 / 25 are odd, so the DATA would
// do without it, but the twiddle reads tw[r k N / (R Ns)] have strides with the factor 16 of N in them: unpadded, the 25
// distinct twiddles of the radix-5 pass at Ns = 48 of 1200 fall into 8 of the 32 eight-byte slots a 32-lane ds_read_b64 group
// sees (4-way), and in the orders that run the odd radices first all of a group's twiddles share ONE slot (5- and 25-way).
// Worst distinct addresses per slot with the pad (32-lane groups / 32 slots for the 8-byte reads, 16-lane groups / 16 slots
// for the 8-byte writes; tools/fft_lds_conflicts.py prints the table), per pass as (radix, Ns): data read / twiddle / write
//   1200 = 8 * 6 * 5 * 5 : (8, 1) 2 / - / 2   (6, 8) 2 / 2 / 2   (5, 48) 2 / 3 / 1   (5, 240) 2 / 2 / 1
//    400 = 8 * 2 * 5 * 5 : (8, 1) 2 / - / 2   (2, 8) 2 / 2 / 2   (5, 16) 2 / 2 / 1   (5, 80)  2 / 2 / 1
//    240 = 8 * 6 * 5     : (8, 1) 1 / - / 2   (6, 8) 2 / 2 / 2   (5, 48) 2 / 2 / 1
//   2048 = 8 * 8 * 8 * 4 : (8, 1) 1 / - / 2   (8, 8) 1 / 1 / 2   (8, 64) 1 / 2 / 1   (4, 512) 1 / 2 / 1   (for comparison)
// The 2-way data reads of the mixed sizes: N / R is no multiple of 32, so a group's 32 contiguous elements straddle one pad
// step and its last element lands on the slot of its first (one extra LDS cycle per read).  A 2-way 8-byte write costs
// nothing (the store's cycles are set by moving its operands to the LDS, not by the array).  A pad of i + (i >> 4) is worse
// on every size (8-way twiddles at (5, 48)); no pad at all is 8-way on the first pass's writes.
__device__ __forceinline__ int fpad(int i) { return i + (i >> 5); }
template <int N>
struct FftLds {
  static constexpr int SIZE = N + N / 32 + 1;
  static constexpr bool POW2 = (N & (N - 1)) == 0;
  static constexpr int PN = (N + 255) / 256;  // elements per thread (the last one guarded unless 256 divides N)
  // index of the Hermitian partner of bin k: (N - k) mod N
  static __device__ __forceinline__ int neg(int k) {
    if constexpr (POW2) return (N - k) & (N - 1);
    else return k ? N - k : 0;
  }
};

// in-place complex FFT of the padded LDS array buf (logical 0 .. N), 256 threads; tw (padded) logical j = exp(-2 pi i j / N);
// INV: conjugate transform (unscaled).  Stockham autosort passes of radix 8 while a factor 8 is left, then one radix-4 or
// radix-2 pass (2048 = 8 * 8 * 8 * 4: FOUR LDS round trips; the first form of this kernel ran five radix-4 passes and a
// radix-2 one with run-time strides).  Pass with Ns done: butterfly j (0 .. N / R) reads x_r = buf[j + r N / R] * w^(r k)
// with k = j mod Ns, w = exp(-+2 pi i / (R Ns)), and writes its R outputs to (j - k) R + k + s Ns -- for ANY radix sequence.
// The plan of a size is fft_radix() applied to what is left: 8, else 6 (= 2 x 3), 4, 2 while the rest is even, then 5 and 3.
// 1200 = 8 * 6 * 5 * 5 is FOUR round trips (4 * 4 * 3 * 5 * 5 would be five); the even radices go FIRST because (a) that is the
// order the power-of-two plans already have, so one rule serves all sizes and theirs is unchanged, (b) the radix-5 passes,
// which keep 240 of the 256 threads busy at 1200 (radix 8: 150), then run with Ns = 48 and 240, where their writes are
// contiguous runs, and (c) of the four-pass orders it has the fewest modelled LDS cycles (table above: 94 against 99 for
// 5 * 5 * 6 * 8 and 97 - 105 for the interleaved ones, all within the model's error -- no order is clearly better).
constexpr int fft_radix(int rest) {
  return rest % 8 == 0 ? 8 : rest % 6 == 0 ? 6 : rest % 4 == 0 ? 4 : rest % 2 == 0 ? 2 : rest % 5 == 0 ? 5 : rest % 3 == 0 ? 3 : 0;
}
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
  } else if constexpr (R == 3) {
    // X_0 = x_0 + a ; X_1,2 = x_0 - a / 2 -+ i (sqrt 3 / 2) b with a = x_1 + x_2, b = x_1 - x_2 (INV: +-)
    constexpr float h3 = 0.86602540378443864676f;
    const cplx a = cadd(v[1], v[2]), b = csub(v[1], v[2]);
    const cplx t = cplx{v[0].x - 0.5f * a.x, v[0].y - 0.5f * a.y}, u = mul_mi<INV>(cplx{h3 * b.x, h3 * b.y});
    v[0] = cadd(v[0], a);
    v[1] = cadd(t, u);
    v[2] = csub(t, u);
  } else if constexpr (R == 5) {
    // a_n = x_n + x_{5-n}, b_n = x_n - x_{5-n}: X_1,4 = x_0 + c1 a_1 + c2 a_2 -+ i (s1 b_1 + s2 b_2),
    // X_2,3 = x_0 + c2 a_1 + c1 a_2 -+ i (s2 b_1 - s1 b_2) with c_n + i s_n = exp(2 pi i n / 5) (INV: +-)
    constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
    constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
    const cplx a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]), b1 = csub(v[1], v[4]), b2 = csub(v[2], v[3]);
    const cplx t1 = cplx{v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y};
    const cplx t2 = cplx{v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y};
    const cplx u1 = mul_mi<INV>(cplx{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y});
    const cplx u2 = mul_mi<INV>(cplx{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y});
    v[0] = cadd(v[0], cadd(a1, a2));
    v[1] = cadd(t1, u1);
    v[2] = cadd(t2, u2);
    v[3] = csub(t2, u2);
    v[4] = csub(t1, u1);
  } else if constexpr (R == 6) {
    // X_k, X_{k+3} = E_k +- w6^k O_k: E, O the 3-point transforms of the even and the odd inputs
    constexpr float h3 = 0.86602540378443864676f;
    cplx e[3] = {v[0], v[2], v[4]}, o[3] = {v[1], v[3], v[5]};
    dft_small<3, INV>(e);
    dft_small<3, INV>(o);
    o[1] = cmul(o[1], cplx{0.5f, INV ? h3 : -h3});
    o[2] = cmul(o[2], cplx{-0.5f, INV ? h3 : -h3});
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      v[q] = cadd(e[q], o[q]);
      v[q + 3] = csub(e[q], o[q]);
    }
  } else if constexpr (R == 4) {
    const cplx e0 = cadd(v[0], v[2]), e1 = csub(v[0], v[2]), e2 = cadd(v[1], v[3]), e3 = mul_mi<INV>(csub(v[1], v[3]));
    v[0] = cadd(e0, e2);
    v[1] = cadd(e1, e3);
    v[2] = csub(e0, e2);
    v[3] = csub(e1, e3);
  } else {
    static_assert(R == 8, "no butterfly of this radix");
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
template <int NS>
__device__ __forceinline__ int fft_mod(int j) {  // j mod NS, j >= 0
  if constexpr ((NS & (NS - 1)) == 0) return j & (NS - 1);
  else return j % NS;
}
template <int N, int NS, int R, bool INV>
__device__ __forceinline__ void fft_pass(cplx* buf, const cplx* tw, int tid) {
  static_assert(N % (R * NS) == 0, "the radix plan does not divide N");
  constexpr int NB = N / R, PER = (NB + 255) / 256, TS = N / (R * NS);
  cplx v[PER][R];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int j = tid + 256 * i;
    if (NB % 256 == 0 || j < NB) {
      const int k = fft_mod<NS>(j);
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
      const int k = fft_mod<NS>(j);
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
    constexpr int R = fft_radix(N / NS);
    static_assert(R > 0, "N has a prime factor above 5");
    fft_pass<N, NS, R, INV>(buf, tw, tid);
    fft_passes<N, NS * R, INV>(buf, tw, tid);
  }
}
template <int N, bool INV>
__device__ void fft_lds(cplx* buf, const cplx* tw, int tid) {
  fft_passes<N, 1, INV>(buf, tw, tid);
}

}  // namespace
