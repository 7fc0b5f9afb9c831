// Griffin-Lim vocoder kernels (config 5): the log-mel -> magnitude glue, the dense-DFT form on the bf16 matrix cores and
// the real-FFT form in LDS.
//
// Reference call sites replaced: fairseq/models/text_to_speech/vocoder.py:84-144 + fairseq/data/audio/audio_utils.py:259-271
// (Griffin-Lim: polar <-> rectangular spectra around the STFT / inverse STFT, overlap-add; exp and clamp around the
// pseudo-inverse mel GEMM).
#include "s2st_ops.h"
#include "s2st_prof.h"
#include "fft_lds.h"

namespace {

// y[c][t] = exp(x[t][c])   (vocoder.py:139: x.exp().transpose(-1, -2))
__global__ __launch_bounds__(256) void exp_transpose_kernel(const float* __restrict__ x, float* __restrict__ y, int T,
                                                            int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)T * C) return;
  const int c = (int)(i / T), t = (int)(i - (long)c * T);
  y[i] = expf(x[(long)t * C + c]);
}
__global__ __launch_bounds__(256) void exp_kernel(float* __restrict__ x, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = expf(x[i]);
}
__global__ __launch_bounds__(256) void clamp_min_kernel(float* __restrict__ x, long n, float lo) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) x[i] = fmaxf(x[i], lo);
}

// ---- batched Griffin-Lim on the bf16 matrix cores: U utterances with T_u = tl[u] <= Tmax frames, rows
// r = u * Tmax + t.  The dense-DFT GEMMs run as ONE bf16 GEMM each with the bf16x3 split folded into the
// contraction dimension: an fp32 row x (K values) is stored as the bf16 row [hi(x) | lo(x) | hi(x)] (3K) and
// the constant basis as [hi(b) | hi(b) | lo(b)], so the MFMA chain accumulates hi*hi + lo*hi + hi*lo in
// fp32 (~2^-17 relative, the accuracy of the fp32-operand "precise" GEMM) at the bf16 kernel's speed.
// Spectra are [rows][re(0..F) pad | im(0..F) pad] with the halves Fp = roundup(F, 16) apart; frames
// t >= T_u and pad columns are written as zeros.
__device__ __forceinline__ void store_split4(uint16_t* dst, long seg, const float v[4]) {
  uint2 hi, lo;
  split_bf16x4(v[0], v[1], v[2], v[3], hi, lo);
  *reinterpret_cast<uint2*>(dst) = hi;
  *reinterpret_cast<uint2*>(dst + seg) = lo;
  *reinterpret_cast<uint2*>(dst + 2 * seg) = hi;
}
// MODE 0: X = mag * exp(i ang) from the initial angles (aux = ang [rows][F]);
// MODE 1: X = mag * exp(i angle(Y)) from the re-analysed spectrum (aux = Y [rows][2 Fp])
template <int MODE>
__global__ __launch_bounds__(256) void gl_polar_split_kernel(const float* __restrict__ mag, const float* __restrict__ aux,
                                                             const int* __restrict__ tl, uint16_t* __restrict__ Xs,
                                                             int U, int F, int Fp, int Tmax) {
  const int q = Fp / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * Tmax * q) return;
  const int f4 = (int)(i % q) * 4;
  const long row = i / q;
  const int t = (int)(row % Tmax), u = (int)(row / Tmax);
  float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
  if (t < tl[u]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int f = f4 + e;
      if (f < F) {
        const float m = mag[row * F + f];
        const float a = MODE == 0 ? aux[row * F + f] : atan2f(aux[row * 2 * Fp + Fp + f], aux[row * 2 * Fp + f]);
        re[e] = m * cosf(a);
        im[e] = m * sinf(a);
      }
    }
  }
  uint16_t* xr = Xs + row * 6 * Fp;
  store_split4(xr + f4, 2 * Fp, re);
  store_split4(xr + Fp + f4, 2 * Fp, im);
}
// analysis frames of the reflect-padded waveforms, split for the STFT GEMM: As[row][3][n_fft]
__global__ __launch_bounds__(256) void gl_frame_split_kernel(const float* __restrict__ wave, const int* __restrict__ tl,
                                                             uint16_t* __restrict__ As, int U, int Tmax, int hop,
                                                             int n_fft, int Lw) {
  const int q = n_fft / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * Tmax * q) return;
  const int j4 = (int)(i % q) * 4;
  const long row = i / q;
  const int t = (int)(row % Tmax), u = (int)(row / Tmax);
  const int T = tl[u], n = hop * (T - 1), pad = n_fft / 2;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (t < T && n > pad) {
    const float* w = wave + (long)u * Lw;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int j = t * hop + j4 + e - pad;
      if (j < 0) j = -j;
      if (j >= n) j = 2 * (n - 1) - j;
      v[e] = w[j];
    }
  }
  store_split4(As + row * 3 * n_fft + j4, n_fft, v);
}
// per-utterance overlap-add of frames[u][t < T_u][n_fft]; wsq[T][..] is looked up per T_u through wsq_off
__global__ __launch_bounds__(256) void gl_overlap_add_b_kernel(const float* __restrict__ frames,
                                                               const float* __restrict__ wsq_all,
                                                               const long* __restrict__ wsq_off,
                                                               const int* __restrict__ tl, float* __restrict__ wave,
                                                               int U, int Tmax, int n_fft, int hop, int Lw, float tiny) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * Lw) return;
  const int u = (int)(i / Lw), q = (int)(i - (long)u * Lw);
  const int T = tl[u];
  float out = 0.f;
  if (q < hop * (T - 1)) {
    const int pos = q + n_fft / 2;
    int t1 = pos / hop;
    if (t1 > T - 1) t1 = T - 1;
    const int t0 = pos - n_fft + 1 <= 0 ? 0 : (pos - n_fft + 1 + hop - 1) / hop;
    float a = 0.f;
    for (int t = t0; t <= t1; ++t) a += frames[((long)u * Tmax + t) * n_fft + (pos - t * hop)];
    const float w = wsq_all[wsq_off[u] + pos];
    if (w > tiny) a /= w;
    out = a * ((float)n_fft / (float)hop);
  }
  wave[i] = out;
}

// ------------------------------------------------------------------------------------------------
// Griffin-Lim with FFTs (round 4).  The reference's STFT / inverse STFT are dense Fourier-basis convolutions
// (audio_utils.py:226-271: basis = [Re; Im] of fft(eye(n_fft)) * window; vocoder.py:56-98: pinverse(n_fft / hop * basis)):
//   * the analysis is exactly rfft(window * frame);
//   * the synthesis basis pinverse(s B)^T equals the plain inverse real FFT / s: B^T B = (N/2) I + E with E[n][m] = 1 for
//     n - m even, whose inverse turns B^T X = Re sum_{k <= N/2} X_k W^{kn} into (1/N) [X_0 + X_{N/2} (-1)^n + 2 sum_{0<k<N/2}
//     Re X_k W^{kn}] (imaginary parts of the DC and Nyquist bins dropped) -- checked numerically against numpy's pinv to 1e-16.
// So both directions are N-point real FFTs: O(N log N) per frame instead of the 2 N (N + 2) multiply-adds of the dense
// contraction (x 3 in the bf16x3 GEMM form that rounds 1 - 3 used: 137 ms of the 237 ms one 16-utterance batch took).
// One workgroup transforms TWO frames at once as the real and imaginary part of one complex N-point FFT (Stockham
// autosort in LDS, fft_lds.h: 8 N bytes + the twiddle table) and separates / merges the two spectra through the Hermitian
// symmetry.  N = 256 ... 2048 (powers of two) and the mixed-radix sizes 240, 400, 1200; other n_fft keep the GEMM path.
// ------------------------------------------------------------------------------------------------
// (cplx, fpad, FftLds<N> and fft_lds<N, INV>: fft_lds.h, shared with features.hip)

// STFT of the reflect-padded waveforms + phase projection, per PAIR of frames (rows m0 = 2 * pair, m0 + 1 of the
// flattened [U][Tmax] frame index): X[m][k] = mag[m][k] * Y_k / |Y_k| with Y = rfft(window * frame) -- the reference's
// mag * (cos, sin)(atan2(Im Y, Re Y)) (audio_utils.py:259-271, vocoder.py:104-107; |Y| = 0: angle 0).  Rows t >= T_u: zeros.
// A workgroup walks several pairs; the NEXT pair's samples and this pair's magnitudes are fetched into registers before
// the transform starts, so the memory round trips run under the butterflies (first version: load -> transform -> load ->
// store in sequence, ~18 us per pair and workgroup with four workgroups per CU).
// Which two rows share a transform: rows 2 * pair, 2 * pair + 1 of the flattened index (a pair may span two utterances) --
// or, PER_UTT (gl_istft_frames_kernel at the mixed-radix N), frames (2 p, 2 p + 1) of ONE utterance, pair = u * ceil(Tmax / 2)
// + p: the pairs the one-launch inverse (gl_istft_ola_kernel, which starts its blocks at even frames for these N) forms too,
// so that the two inverse forms give the same bits: a packed transform's rounding depends on both halves (1e-7 of the frame scale), and the phase
// projection of the next iteration amplifies that (measured 2e-6 of the waveform scale after three iterations at 240).
template <int N, bool PER_UTT = false>
struct PairInfo {
  int tt[2], uu[2], TT[2];
  bool on[2];
  // row of half h of a pair in the flattened [U][Tmax] index; has(): the row exists
  static __device__ __forceinline__ long row(long pair, int h, int Tmax) {
    if constexpr (!PER_UTT) return 2 * pair + h;
    else {
      const int PT = (Tmax + 1) / 2;
      return (pair / PT) * Tmax + 2 * (pair % PT) + h;
    }
  }
  static __device__ __forceinline__ bool has(long pair, int h, long M, int Tmax) {
    if constexpr (!PER_UTT) return 2 * pair + h < M;
    else return 2 * (pair % ((Tmax + 1) / 2)) + h < Tmax;
  }
  __device__ __forceinline__ void set(long pair, long M, int Tmax, const int* tl, int hop, bool need_len) {
    for (int h = 0; h < 2; ++h) {
      const long m = row(pair, h, Tmax);
      const bool in = has(pair, h, M, Tmax);
      uu[h] = in ? (int)(m / Tmax) : 0;
      tt[h] = in ? (int)(m - (long)uu[h] * Tmax) : 0;
      TT[h] = tl[uu[h]];
      on[h] = in && tt[h] < TT[h] && (!need_len || hop * (TT[h] - 1) > N / 2);
    }
  }
};

template <int N>
__global__ __launch_bounds__(256) void gl_stft_project_kernel(const float* __restrict__ wave, const int* __restrict__ tl,
                                                              const float* __restrict__ win, const cplx* __restrict__ twg,
                                                              const float* __restrict__ mag, cplx* __restrict__ X, int U,
                                                              int Tmax, int hop, int Lw, long npairs) {
  __shared__ cplx buf[FftLds<N>::SIZE];
  __shared__ cplx tw[FftLds<N>::SIZE];
  const int tid = threadIdx.x;
  constexpr int F = N / 2 + 1, PN = FftLds<N>::PN, PF = (F + 255) / 256;
  for (int j = tid; j < N; j += 256) tw[fpad(j)] = twg[j];
  const long M = (long)U * Tmax;
  float wn[PN];
#pragma unroll
  for (int i = 0; i < PN; ++i) wn[i] = (N % 256 == 0 || tid + 256 * i < N) ? win[tid + 256 * i] : 0.f;
  cplx xr[PN];
  auto fetch = [&](const PairInfo<N>& pi) {
#pragma unroll
    for (int i = 0; i < PN; ++i) {
      const int n = tid + 256 * i;
      float v[2] = {0.f, 0.f};
      for (int h = 0; h < 2; ++h) {
        if (!pi.on[h] || (N % 256 != 0 && n >= N)) continue;
        const int len = hop * (pi.TT[h] - 1);
        int j = pi.tt[h] * hop + n - N / 2;
        if (j < 0) j = -j;
        if (j >= len) j = 2 * (len - 1) - j;
        v[h] = wave[(long)pi.uu[h] * Lw + j];
      }
      xr[i] = cplx{v[0] * wn[i], v[1] * wn[i]};
    }
  };
  PairInfo<N> cur, nxt;
  long pair = blockIdx.x;
  if (pair < npairs) {
    cur.set(pair, M, Tmax, tl, hop, true);
    fetch(cur);
  }
  for (; pair < npairs; pair += gridDim.x) {
    const long m0 = 2 * pair;
    __syncthreads();  // (the previous pair's readers are done with buf)
#pragma unroll
    for (int i = 0; i < PN; ++i)
      if (N % 256 == 0 || tid + 256 * i < N) buf[fpad(tid + 256 * i)] = xr[i];
    // this pair's magnitudes and the next pair's samples: in flight during the transform
    float mg[PF][2];
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      for (int h = 0; h < 2; ++h) mg[i][h] = (k < F && cur.on[h]) ? mag[(m0 + h) * F + k] : 0.f;
    }
    const long np_ = pair + gridDim.x;
    if (np_ < npairs) {
      nxt.set(np_, M, Tmax, tl, hop, true);
      fetch(nxt);
    }
    __syncthreads();
    fft_lds<N, false>(buf, tw, tid);
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      if (k >= F) continue;
      const cplx zk = buf[fpad(k)], zn = buf[fpad(FftLds<N>::neg(k))];
      // Y1 = (Z_k + conj Z_{N-k}) / 2 ; Y2 = (Z_k - conj Z_{N-k}) / (2 i)
      const cplx y[2] = {cplx{0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)}, cplx{0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)}};
      for (int h = 0; h < 2; ++h) {
        const long m = m0 + h;
        if (m >= M) continue;
        cplx o{0.f, 0.f};
        if (cur.on[h]) {
          const float a2 = y[h].x * y[h].x + y[h].y * y[h].y;
          if (a2 > 0.f) {
            const float r = mg[i][h] * rsqrtf(a2);
            o = cplx{y[h].x * r, y[h].y * r};
          } else {
            o = cplx{mg[i][h], 0.f};
          }
        }
        X[m * F + k] = o;
      }
    }
    cur = nxt;
  }
}

template <int N>
using FramePairs = PairInfo<N, !FftLds<N>::POW2>;

// inverse: frames[m][n] = window[n] * (hop / N) * irfft(X[m])[n] for the two rows of a pair (rows t >= T_u: zeros);
// the overlap-add kernel above turns the frames into the waveforms.  The next pair's spectra are fetched ahead likewise.
template <int N>
__global__ __launch_bounds__(256) void gl_istft_frames_kernel(const cplx* __restrict__ X, const int* __restrict__ tl,
                                                              const float* __restrict__ win, const cplx* __restrict__ twg,
                                                              float* __restrict__ frames, int U, int Tmax, int hop, long npairs) {
  __shared__ cplx buf[FftLds<N>::SIZE];
  __shared__ cplx tw[FftLds<N>::SIZE];
  const int tid = threadIdx.x;
  constexpr int F = N / 2 + 1, PN = FftLds<N>::PN, PF = (F + 255) / 256;
  for (int j = tid; j < N; j += 256) tw[fpad(j)] = twg[j];
  const float sc = (float)hop / ((float)N * (float)N);
  const long M = (long)U * Tmax;
  float wn[PN];
#pragma unroll
  for (int i = 0; i < PN; ++i) wn[i] = (N % 256 == 0 || tid + 256 * i < N) ? win[tid + 256 * i] * sc : 0.f;
  cplx xa[PF], xb[PF];
  auto fetch = [&](const FramePairs<N>& pi, long m0) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      xa[i] = (k < F && pi.on[0]) ? X[m0 * F + k] : cplx{0.f, 0.f};
      xb[i] = (k < F && pi.on[1]) ? X[(m0 + 1) * F + k] : cplx{0.f, 0.f};
    }
  };
  FramePairs<N> cur, nxt;
  long pair = blockIdx.x;
  if (pair < npairs) {
    cur.set(pair, M, Tmax, tl, hop, false);
    fetch(cur, FramePairs<N>::row(pair, 0, Tmax));
  }
  for (; pair < npairs; pair += gridDim.x) {
    const long m0 = FramePairs<N>::row(pair, 0, Tmax);  // (the pair's second row is m0 + 1)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      if (k >= F) continue;
      cplx a = xa[i], b = xb[i];
      if (k == 0 || k == N / 2) a.y = b.y = 0.f;  // (the basis' sine rows of DC / Nyquist are zero)
      buf[fpad(k)] = cplx{a.x - b.y, a.y + b.x};                             // Z_k     = X1_k + i X2_k
      if (k > 0 && k < N / 2) buf[fpad(N - k)] = cplx{a.x + b.y, b.x - a.y};  // Z_{N-k} = conj X1_k + i conj X2_k
    }
    const long np_ = pair + gridDim.x;
    if (np_ < npairs) {
      nxt.set(np_, M, Tmax, tl, hop, false);
      fetch(nxt, FramePairs<N>::row(np_, 0, Tmax));
    }
    __syncthreads();
    fft_lds<N, true>(buf, tw, tid);
#pragma unroll
    for (int i = 0; i < PN; ++i) {
      const int n = tid + 256 * i;
      if (N % 256 != 0 && n >= N) continue;
      const cplx z = buf[fpad(n)];
      if (FramePairs<N>::has(pair, 0, M, Tmax)) frames[m0 * N + n] = cur.on[0] ? z.x * wn[i] : 0.f;
      if (FramePairs<N>::has(pair, 1, M, Tmax)) frames[(m0 + 1) * N + n] = cur.on[1] ? z.y * wn[i] : 0.f;
    }
    cur = nxt;
  }
}

// inverse transform AND overlap-add in one launch (the 367 MB of synthesis frames per iteration -- written by the kernel
// above, read back by gl_overlap_add_b -- never exist).  Workgroup (b, u) owns the output samples q in [b S, (b + 1) S) of
// utterance u (S = R hops) and inverse-transforms every frame that touches them in ascending order: its own R frames plus
// the ceil(N / hop) in front whose tails reach in (recomputed by the neighbouring workgroup too: +11 % transforms at R = 64
// for n_fft 2048 / hop 300).  The accumulator is a CIRCULAR LDS array of C >= N + 2 hop floats (a power of two): once a pair
// (t, t + 1) is added, the samples in front of (t + 2) hop are final -- they are normalised, written out and their slots
// cleared for the samples C further on.  (First form: an S-float accumulator, 72 KB of LDS per workgroup, two workgroups per
// CU: 329 us per launch against 136 + 164 for the two-kernel form; the transforms are latency-bound and want 3 - 4
// workgroups per CU.)  Frames are added in ascending order with a barrier between the two frames of a pair, so every sample
// sees the additions the stand-alone overlap-add makes, in its order (which two frames share a complex transform differs
// from the kernel above, so a frame's last bits can: 1e-8 relative, tests/test_inference.py -- at the power-of-two N; at
// the mixed-radix N both kernels pair frames (2 p, 2 p + 1) of an utterance and give the same bits, see PairInfo).
template <int N>
__global__ __launch_bounds__(256) void gl_istft_ola_kernel(const cplx* __restrict__ X, const int* __restrict__ tl,
                                                           const float* __restrict__ win, const cplx* __restrict__ twg,
                                                           const float* __restrict__ wsq_all, const long* __restrict__ wsq_off,
                                                           float* __restrict__ wave, int Tmax, int hop, int Lw, int S, int C,
                                                           float tiny) {
  HIP_DYNAMIC_SHARED(unsigned char, smem)
  cplx* buf = reinterpret_cast<cplx*>(smem);
  cplx* tw = buf + FftLds<N>::SIZE;
  float* acc = reinterpret_cast<float*>(tw + FftLds<N>::SIZE);
  const int tid = threadIdx.x, u = blockIdx.y;
  constexpr int F = N / 2 + 1, PN = FftLds<N>::PN, PF = (F + 255) / 256;
  const int T = tl[u];
  const int q0 = blockIdx.x * S, q1 = min(q0 + S, Lw);
  const int len = hop * (T - 1);  // samples of this utterance (vocoder.py:95-97: the n_fft / 2 borders are trimmed)
  float* out = wave + (long)u * Lw;
  if (q0 >= len) {
    for (int q = q0 + tid; q < q1; q += 256) out[q] = 0.f;
    return;
  }
  for (int q = max(q0, len) + tid; q < q1; q += 256) out[q] = 0.f;  // (behind the utterance's end)
  for (int j = tid; j < N; j += 256) tw[fpad(j)] = twg[j];
  for (int i = tid; i < C; i += 256) acc[i] = 0.f;
  const int cm = C - 1;
  const float sc = (float)hop / ((float)N * (float)N);
  float wn[PN];
#pragma unroll
  for (int i = 0; i < PN; ++i) wn[i] = (N % 256 == 0 || tid + 256 * i < N) ? win[tid + 256 * i] * sc : 0.f;
  const int P0 = q0 + N / 2, P1 = min(q1, len) + N / 2;  // owned positions of the untrimmed signal
  const int t_lo = P0 - N + 1 <= 0 ? 0 : (P0 - N + hop) / hop;
  // mixed sizes: the pairs of gl_istft_frames_kernel, (2 p, 2 p + 1) of the utterance -- start at an even frame (an odd first
  // frame's predecessor ends in front of P0: its samples are dropped by the flush) and give a frame its real partner even
  // when that lies beyond the block (transformed, not added); see PairInfo
  const int t_beg = FftLds<N>::POW2 ? t_lo : (t_lo & ~1);
  const int t_hi = min(T - 1, (P1 - 1) / hop);
  const cplx* Xu = X + (long)u * Tmax * F;
  const float* wsq = wsq_all + wsq_off[u];
  const float gain = (float)N / (float)hop;
  cplx xa[PF], xb[PF];
  auto fetch = [&](int t) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      xa[i] = (k < F && t <= t_hi) ? Xu[(long)t * F + k] : cplx{0.f, 0.f};
      if constexpr (FftLds<N>::POW2)
        xb[i] = (k < F && t + 1 <= t_hi) ? Xu[(long)(t + 1) * F + k] : cplx{0.f, 0.f};
      else  // (the real partner, also beyond the block)
        xb[i] = (k < F && t + 1 < T) ? Xu[(long)(t + 1) * F + k] : cplx{0.f, 0.f};
    }
  };
  fetch(t_beg);
  int done = t_beg * hop;  // positions in front of `done` are final and flushed
  for (int t = t_beg; t <= t_hi; t += 2) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      const int k = tid + 256 * i;
      if (k >= F) continue;
      cplx a = xa[i], b = xb[i];
      if (k == 0 || k == N / 2) a.y = b.y = 0.f;
      buf[fpad(k)] = cplx{a.x - b.y, a.y + b.x};
      if (k > 0 && k < N / 2) buf[fpad(N - k)] = cplx{a.x + b.y, b.x - a.y};
    }
    if (t + 2 <= t_hi) fetch(t + 2);
    __syncthreads();
    fft_lds<N, true>(buf, tw, tid);
    float zx[PN], zy[PN];
    {
#pragma clang fp contract(off)  // (product rounded, then added: what the frames-through-HBM form does; no fused multiply-add)
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        if (N % 256 != 0 && tid + 256 * i >= N) continue;
        const cplx z = buf[fpad(tid + 256 * i)];
        zx[i] = z.x * wn[i];
        zy[i] = z.y * wn[i];
      }
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        if (N % 256 != 0 && tid + 256 * i >= N) continue;
        const int sl = (t * hop + tid + 256 * i) & cm;
        acc[sl] = acc[sl] + zx[i];
      }
    }
    __syncthreads();
    if (t + 1 <= t_hi) {
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        if (N % 256 != 0 && tid + 256 * i >= N) continue;
        const int sl = ((t + 1) * hop + tid + 256 * i) & cm;
        acc[sl] = acc[sl] + zy[i];
      }
    }
    __syncthreads();
    // final now: everything in front of the next pair's first position (after the last pair: up to the block's end)
    const int upto = t + 2 <= t_hi ? (t + 2) * hop : P1;
    for (int p = done + tid; p < upto; p += 256) {
      const int sl = p & cm;
      if (p >= P0 && p < P1) {
        float a = acc[sl];
        const float w = wsq[p];
        if (w > tiny) a /= w;
        out[p - N / 2] = a * gain;
      }
      acc[sl] = 0.f;
    }
    done = upto;
  }
}

// The initial phases on the device.  The reference draws np.random.rand(F, T_u) per utterance from numpy's global generator and
// takes np.angle(np.exp(2j pi u)) (vocoder.py:101-102) = 2 pi u wrapped into (-pi, pi], in double, then casts to the
// spectrogram's dtype.  `uni`: those uniform draws, as drawn (utterance u's [F][T_u] block at uni + uoff[u]): the wrap, the
// cast, the transposition to frame-major and mag * (cos, sin) happen here (the host only runs the generator -- rounds 1 - 3
// also wrapped, cast and transposed 45 M numbers per 64 utterances there: 2/3 of the vocoder's wall time).  uni == nullptr:
// the draws themselves come from the counter-based hash of (seed, utterance, bin, frame) -- same distribution, not numpy's
// stream (GriffinLim(phase_rng="device")).  One thread per (u, k, t), t fastest: coalesced reads of uni.
__global__ __launch_bounds__(256) void gl_polar_u_kernel(const float* __restrict__ mag, const double* __restrict__ uni,
                                                         const long* __restrict__ uoff, const int* __restrict__ tl,
                                                         uint64_t seed, cplx* __restrict__ X, int U, int F, int Tmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * F * Tmax) return;
  const int t = (int)(i % Tmax);
  const long r = i / Tmax;
  const int k = (int)(r % F), u = (int)(r / F);
  const int T = tl[u];
  cplx o{0.f, 0.f};
  if (t < T) {
    double un;
    if (uni) un = uni[uoff[u] + (long)k * T + t];
    else un = (double)(mix32(seed + (uint64_t)u, (uint64_t)k * (uint64_t)Tmax + (uint64_t)t) >> 8) * (1.0 / 16777216.0);
    double a = 6.283185307179586476925286766559 * un;
    if (a > 3.141592653589793238462643383279) a -= 6.283185307179586476925286766559;
    const float af = (float)a, m = mag[((long)u * Tmax + t) * F + k];
    o = cplx{m * cosf(af), m * sinf(af)};
  }
  X[((long)u * Tmax + t) * F + k] = o;
}

// X[m][k] = mag[m][k] * (cos, sin)(ang[m][k]) (the initial phases, vocoder.py:101-103); rows t >= T_u: zeros
__global__ __launch_bounds__(256) void gl_polar_c_kernel(const float* __restrict__ mag, const float* __restrict__ ang,
                                                         const int* __restrict__ tl, cplx* __restrict__ X, int U, int F, int Tmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)U * Tmax * F) return;
  const long row = i / F;
  const int t = (int)(row % Tmax), u = (int)(row / Tmax);
  cplx o{0.f, 0.f};
  if (t < tl[u]) {
    const float m = mag[i], a = ang[i];
    o = cplx{m * cosf(a), m * sinf(a)};
  }
  X[i] = o;
}

}  // namespace

int s2st_exp_transpose(const float* x, float* y, int T, int C, hipStream_t st) {
  const long n = (long)T * C;
  if (n <= 0) return 0;
  S2ST_LAUNCH(exp_transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, T, C);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
int s2st_clamp_min(float* x, long n, float lo, hipStream_t st) {
  if (n <= 0) return 0;
  S2ST_LAUNCH(clamp_min_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n, lo);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_gl_polar_split(const float* mag, const float* aux, int from_spectrum, const int* tl, uint16_t* Xs, int U, int F,
                        int Fp, int Tmax, hipStream_t st) {
  if (Fp % 4 || Fp < F) return S2ST_ERR_SHAPE;
  const long n = (long)U * Tmax * (Fp / 4);
  if (n <= 0) return 0;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (from_spectrum)
    S2ST_LAUNCH(gl_polar_split_kernel<1>, grid, dim3(256), 0, st, mag, aux, tl, Xs, U, F, Fp, Tmax);
  else
    S2ST_LAUNCH(gl_polar_split_kernel<0>, grid, dim3(256), 0, st, mag, aux, tl, Xs, U, F, Fp, Tmax);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
int s2st_gl_frame_split(const float* wave, const int* tl, uint16_t* As, int U, int Tmax, int hop, int n_fft, int Lw,
                        hipStream_t st) {
  if (n_fft % 4) return S2ST_ERR_SHAPE;
  const long n = (long)U * Tmax * (n_fft / 4);
  if (n <= 0) return 0;
  S2ST_LAUNCH(gl_frame_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wave, tl, As, U, Tmax,
                     hop, n_fft, Lw);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
int s2st_gl_overlap_add_b(const float* frames, const float* wsq_all, const long* wsq_off, const int* tl, float* wave,
                          int U, int Tmax, int n_fft, int hop, int Lw, hipStream_t st) {
  const long n = (long)U * Lw;
  if (n <= 0) return 0;
  S2ST_LAUNCH(gl_overlap_add_b_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, frames, wsq_all,
                     wsq_off, tl, wave, U, Tmax, n_fft, hop, Lw, 1.1754944e-38f);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

// ---- FFT-based Griffin-Lim launchers (the n_fft of fft_lds.h's two lists) ---------------------------------------------
#define S2ST_FFT_IS(N) || n_fft == N
// the power-of-two plans (what this query has always meant) / every size fft_lds.h has a plan for
bool s2st_gl_fft_supported(int n_fft) { return false S2ST_FFT_POW2_SIZES(S2ST_FFT_IS); }
bool s2st_fft_len_supported(int n_fft) { return false S2ST_FFT_POW2_SIZES(S2ST_FFT_IS) S2ST_FFT_MIXED_SIZES(S2ST_FFT_IS); }
#undef S2ST_FFT_IS

int s2st_gl_polar_c(const float* mag, const float* ang, const int* tl, float* X, int U, int F, int Tmax, hipStream_t st) {
  const long n = (long)U * Tmax * F;
  if (n <= 0) return 0;
  S2ST_LAUNCH(gl_polar_c_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mag, ang, tl, reinterpret_cast<cplx*>(X), U, F, Tmax);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

// x <- exp(x) in place (the vocoder's log-mel -> mel step, vocoder.py:139, for a whole padded batch at once)
int s2st_exp_inplace(float* x, long n, hipStream_t st) {
  if (n <= 0) return 0;
  S2ST_LAUNCH(exp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, n);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_gl_polar_u(const float* mag, const double* uni, const long* uoff, const int* tl, uint64_t seed, float* X, int U, int F,
                    int Tmax, hipStream_t st) {
  const long n = (long)U * F * Tmax;
  if (n <= 0) return 0;
  if (uni && !uoff) return S2ST_ERR_ARG;
  S2ST_LAUNCH(gl_polar_u_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, mag, uni, uoff, tl, seed,
              reinterpret_cast<cplx*>(X), U, F, Tmax);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

namespace {
template <int N>
int gl_fft_launch(int inverse, const float* wave_or_frames, const int* tl, const float* win, const float* tw, const float* mag,
                  float* X, float* frames, int U, int Tmax, int hop, int Lw, hipStream_t st) {
  // (FramePairs: the inverse transforms of the mixed sizes pair frames within an utterance)
  const long npairs = !inverse || FftLds<N>::POW2 ? ((long)U * Tmax + 1) / 2 : (long)U * ((Tmax + 1) / 2);
  if (npairs <= 0) return 0;
  // (4 k workgroups at most: a workgroup keeps its twiddle table over the pairs it walks)
  const unsigned grid = (unsigned)(npairs < 4096 ? npairs : 4096);
  if (!inverse)
    S2ST_LAUNCH(gl_stft_project_kernel<N>, dim3(grid), dim3(256), 0, st, wave_or_frames, tl, win, reinterpret_cast<const cplx*>(tw),
                mag, reinterpret_cast<cplx*>(X), U, Tmax, hop, Lw, npairs);
  else
    S2ST_LAUNCH(gl_istft_frames_kernel<N>, dim3(grid), dim3(256), 0, st, reinterpret_cast<const cplx*>(X), tl, win,
                reinterpret_cast<const cplx*>(tw), frames, U, Tmax, hop, npairs);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
}  // namespace

// wave [U][Lw] -> X [U * Tmax][n_fft / 2 + 1] complex (re, im interleaved), projected onto the magnitudes mag [U * Tmax][F]
int s2st_gl_stft_project(const float* wave, const int* tl, const float* win, const float* tw, const float* mag, float* X, int U,
                         int Tmax, int n_fft, int hop, int Lw, hipStream_t st) {
#define S2ST_FFT_CASE(N) case N: return gl_fft_launch<N>(0, wave, tl, win, tw, mag, X, nullptr, U, Tmax, hop, Lw, st);
  switch (n_fft) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) S2ST_FFT_MIXED_SIZES(S2ST_FFT_CASE) }
#undef S2ST_FFT_CASE
  return S2ST_ERR_SHAPE;
}

template <int N>
int gl_istft_ola_launch(const float* X, const int* tl, const float* win, const float* tw, const float* wsq_all, const long* wsq_off,
                        float* wave, int U, int Tmax, int hop, int Lw, hipStream_t st) {
  if (U <= 0 || Lw <= 0) return 0;
  if (hop < 1 || hop > N) return S2ST_ERR_ARG;
  // R frames per workgroup: about three workgroups per CU over the batch (S2ST_GL_OLA_FRAMES overrides), at least 16 so that
  // the ceil(N / hop) frames recomputed in front of each block stay a small share
  static const int r_env = [] {
    const char* e = s2st_env_str("S2ST_GL_OLA_FRAMES");
    return e ? atoi(e) : 0;
  }();
  int R = r_env > 0 ? r_env : (int)(((long)U * Tmax + 3 * 256 - 1) / (3 * 256));  // (256 CUs)
  if (R < 16 && r_env <= 0) R = 16;
  if (R > Tmax) R = Tmax;
  if (R < 1) R = 1;
  const int S = R * hop;
  // (a power of two >= N + 2 hop -- for a power-of-two N that is 2 N or 4 N; 2048 floats for 1200 / 300)
  int C = 256;
  while (C < N + 2 * hop) C *= 2;
  const int lds = 2 * FftLds<N>::SIZE * (int)sizeof(cplx) + C * (int)sizeof(float);
  static int configured = 0;  // (per instantiation)
  if (lds > configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(gl_istft_ola_kernel<N>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
        hipSuccess)
      return S2ST_ERR_LAUNCH;
    configured = lds;
  }
  const float tiny = 1.1754944e-38f;
  S2ST_LAUNCH(gl_istft_ola_kernel<N>, dim3((unsigned)((Lw + S - 1) / S), (unsigned)U), dim3(256), lds, st, reinterpret_cast<const cplx*>(X),
              tl, win, reinterpret_cast<const cplx*>(tw), wsq_all, wsq_off, wave, Tmax, hop, Lw, S, C, tiny);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
// X [U * Tmax][F] complex -> wave [U][Lw]: inverse transforms, overlap-add, window-sum-square normalisation, trim (one launch)
int s2st_gl_istft_ola(const float* X, const int* tl, const float* win, const float* tw, const float* wsq_all, const long* wsq_off,
                      float* wave, int U, int Tmax, int n_fft, int hop, int Lw, hipStream_t st) {
#define S2ST_FFT_CASE(N) case N: return gl_istft_ola_launch<N>(X, tl, win, tw, wsq_all, wsq_off, wave, U, Tmax, hop, Lw, st);
  switch (n_fft) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) S2ST_FFT_MIXED_SIZES(S2ST_FFT_CASE) }
#undef S2ST_FFT_CASE
  return S2ST_ERR_ARG;
}
// X [U * Tmax][F] complex -> frames [U * Tmax][n_fft] (windowed synthesis frames; s2st_gl_overlap_add_b finishes)
int s2st_gl_istft_frames(const float* X, const int* tl, const float* win, const float* tw, float* frames, int U, int Tmax,
                         int n_fft, int hop, hipStream_t st) {
#define S2ST_FFT_CASE(N) \
  case N: return gl_fft_launch<N>(1, nullptr, tl, win, tw, nullptr, const_cast<float*>(X), frames, U, Tmax, hop, 0, st);
  switch (n_fft) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) S2ST_FFT_MIXED_SIZES(S2ST_FFT_CASE) }
#undef S2ST_FFT_CASE
  return S2ST_ERR_SHAPE;
}
