// Stage 3 of the recipe on the device: Kaldi filter-bank features of the source audio and log-mel spectrograms of the
// target audio for a ragged batch of utterances, plus the per-utterance moments the global CMVN statistics are made of.
//
// Reference call sites replaced: examples/s2s_trans/preprocessing/get_feature_manifest.py:76-104 --
// examples/speech_to_text/data_utils.py:73-98 (extract_fbank_features -> torchaudio.compliance.kaldi.fbank, restated on the
// host in data/audio_utils.py: kaldi_fbank), examples/speech_synthesis/data_utils.py:46-76 (extract_logmel_spectrogram ->
// TTSSpectrogram + TTSMelScale, fairseq/data/audio/audio_utils.py:218-290) and :190-215 (get_global_cmvn's sums).
//
// Layout shared by all kernels: wave [U][Lmax] fp32 with len[u] valid samples; output rows PACKED, utterance u's T_u frames
// at rows offs[u] .. offs[u + 1]; offs is int32 [2][U + 1]: frame offsets, then PAIR offsets (ceil(T_u / 2) pairs each).
// One workgroup transforms two frames OF ONE UTTERANCE as the real and imaginary part of one complex FFT (fft_lds.h); the
// odd last frame of an utterance is paired with zeros, never with another utterance's frame: the rounding of a packed
// transform depends on both halves, and a frame's result must not depend on what else is in the batch.
// No float atomics; every sum runs in a fixed order.
// For inference from audio files (translate.py) the filter bank also comes as the encoder's input itself: padded
// [U][Tmax][n_bins], global CMVN applied (s2st_fbank_kaldi_batch), and generated waveforms leave as 16-bit PCM (s2st_wave_pcm16).
#include "s2st_ops.h"
#include "s2st_prof.h"
#include "fft_lds.h"

namespace {

// frames of an utterance of n samples.  a, b = (frame size, shift) for the Kaldi framing (snip_edges), (n_fft, hop) for the
// centred, reflect-padded STFT (no frames where torch's reflect padding refuses the input: n <= n_fft / 2)
__device__ __forceinline__ int feat_frames(int n, bool kaldi, int a, int b) {
  if (kaldi) return n < a ? 0 : 1 + (n - a) / b;
  return n <= a / 2 ? 0 : 1 + n / b;
}

// offs[0][u] / offs[1][u]: exclusive sums of T_u / ceil(T_u / 2) (one workgroup: each thread a contiguous run of utterances)
__global__ __launch_bounds__(256) void feat_offsets_kernel(const int* __restrict__ len, int* __restrict__ offs, int U, int kaldi,
                                                           int a, int b) {
  __shared__ int sf[256], sp[256];
  const int tid = threadIdx.x, chunk = (U + 255) / 256;
  const int lo = min(U, tid * chunk), hi = min(U, lo + chunk);
  int f = 0, p = 0;
  for (int u = lo; u < hi; ++u) {
    const int T = feat_frames(len[u], kaldi != 0, a, b);
    f += T;
    p += (T + 1) / 2;
  }
  sf[tid] = f;
  sp[tid] = p;
  __syncthreads();
  if (tid == 0) {
    int af = 0, ap = 0;
    for (int i = 0; i < 256; ++i) {
      const int cf = sf[i], cp = sp[i];
      sf[i] = af;
      sp[i] = ap;
      af += cf;
      ap += cp;
    }
    offs[U] = af;
    offs[2 * U + 1] = ap;
  }
  __syncthreads();
  f = sf[tid];
  p = sp[tid];
  for (int u = lo; u < hi; ++u) {
    const int T = feat_frames(len[u], kaldi != 0, a, b);
    offs[u] = f;
    offs[U + 1 + u] = p;
    f += T;
    p += (T + 1) / 2;
  }
}

// largest u in [0, U) with off[u] <= i (utterances without frames share their successor's offset and are skipped)
__device__ __forceinline__ int feat_find(const int* __restrict__ off, int U, int i) {
  int lo = 0, hi = U;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// frame pair -> window -> fft_lds -> |.|^2 (KALDI) or |.| into LDS -> mel rows over their bin ranges -> log(max(., eps)).
//   KALDI: frames of `size` samples every `hop`, DC removed per frame, pre-emphasis 0.97 (first sample against itself),
//          window[size], zero padding to N.
//   else : frames of N samples every `hop` around the reflect-padded waveform (pad N / 2), window[N].
// mel [n_bins][N / 2 + 1] dense rows; range[b] = {first bin, one past the last bin} of row b: summed in index order.
// BATCH: the epilogue writes the encoder's input instead of packed rows -- frame t of utterance u at row u * Tmax + t of
// out [U][Tmax][n_bins], as (value - cmean[b]) / cstd[b] (an fp32 subtract, then an IEEE fp32 divide: _GlobalCMVN's two numpy
// operations); same pairs, same sums, so `value` has the packed route's bits.  Rows T_u .. Tmax: feat_pad_rows_kernel.
template <int N, bool KALDI, bool BATCH = false>
__global__ __launch_bounds__(256) void feat_fft_kernel(const float* __restrict__ wave, const int* __restrict__ len,
                                                       const float* __restrict__ win, const cplx* __restrict__ twg,
                                                       const float* __restrict__ mel, const int* __restrict__ range,
                                                       float* __restrict__ out, const int* __restrict__ offs, int U, int Lmax,
                                                       int size, int hop, int n_bins, float eps, long out_rows,
                                                       const float* __restrict__ cmean, const float* __restrict__ cstd,
                                                       int Tmax) {
  __shared__ cplx buf[FftLds<N>::SIZE];
  __shared__ cplx tw[FftLds<N>::SIZE];
  __shared__ float sp[2][N / 2 + 1];
  __shared__ float red[8];
  const int tid = threadIdx.x;
  constexpr int F = N / 2 + 1, PN = FftLds<N>::PN, PF = (F + 255) / 256;
  for (int j = tid; j < N; j += 256) tw[fpad(j)] = twg[j];
  float wn[PN];
#pragma unroll
  for (int i = 0; i < PN; ++i) {
    const int n = tid + 256 * i;
    wn[i] = n < size ? win[n] : 0.f;
  }
  // (the value at the clamp, rounded once from double: the device's logf is a couple of ulp off at log(eps))
  const float log_eps = (float)log((double)eps);
  const int* foff = offs;
  const int* poff = offs + U + 1;
  const int npairs = poff[U];
  for (int pair = blockIdx.x; pair < npairs; pair += gridDim.x) {
    const int u = feat_find(poff, U, pair);
    const int t0 = 2 * (pair - poff[u]), T = foff[u + 1] - foff[u], L = len[u];
    const long row0 = BATCH ? (long)u * Tmax + t0 : (long)foff[u] + t0;
    const bool on[2] = {BATCH ? t0 < Tmax : row0 < out_rows, t0 + 1 < T && (BATCH ? t0 + 1 < Tmax : row0 + 1 < out_rows)};
    const float* w = wave + (long)u * Lmax;
    cplx x[PN];
    if (KALDI) {
      float v[PN][2], pv[PN][2], s[2] = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        const int n = tid + 256 * i;
        for (int h = 0; h < 2; ++h) {
          const long j = (long)(t0 + h) * hop + n;
          const bool ok = on[h] && n < size && j < L;
          v[i][h] = ok ? w[j] : 0.f;
          pv[i][h] = ok ? w[n > 0 ? j - 1 : j] : 0.f;
          s[h] += v[i][h];
        }
      }
      for (int h = 0; h < 2; ++h) s[h] = wave_sum(s[h]);
      if ((tid & 63) == 0) {
        red[2 * (tid >> 6)] = s[0];
        red[2 * (tid >> 6) + 1] = s[1];
      }
      __syncthreads();
      const float mean[2] = {((red[0] + red[2]) + (red[4] + red[6])) / (float)size,
                             ((red[1] + red[3]) + (red[5] + red[7])) / (float)size};
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        float y[2];
        for (int h = 0; h < 2; ++h) y[h] = ((v[i][h] - mean[h]) - 0.97f * (pv[i][h] - mean[h])) * wn[i];
        x[i] = cplx{y[0], y[1]};
      }
    } else {
#pragma unroll
      for (int i = 0; i < PN; ++i) {
        const int n = tid + 256 * i;
        float v[2] = {0.f, 0.f};
        for (int h = 0; h < 2; ++h) {
          if (!on[h] || (N % 256 != 0 && n >= N)) continue;
          int j = (t0 + h) * hop + n - N / 2;
          if (j < 0) j = -j;
          if (j >= L) j = 2 * (L - 1) - j;
          v[h] = w[j];
        }
        x[i] = cplx{v[0] * wn[i], v[1] * wn[i]};
      }
    }
#pragma unroll
    for (int i = 0; i < PN; ++i)
      if (N % 256 == 0 || tid + 256 * i < N) buf[fpad(tid + 256 * i)] = x[i];
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
        const float p = y[h].x * y[h].x + y[h].y * y[h].y;
        sp[h][k] = KALDI ? p : sqrtf(p);
      }
    }
    __syncthreads();
    for (int o = tid; o < 2 * n_bins; o += 256) {
      const int h = o / n_bins, b = o - h * n_bins;
      if (!on[h]) continue;
      const float* m = mel + (long)b * F;
      float acc = 0.f;
      for (int k = range[2 * b]; k < range[2 * b + 1]; ++k) acc += sp[h][k] * m[k];
      const float v = acc > eps ? logf(acc) : log_eps;
      out[(row0 + h) * n_bins + b] = BATCH ? (v - cmean[b]) / cstd[b] : v;
    }
    // (the next pair writes buf / red / sp only behind barriers every thread passes after these reads)
    __syncthreads();
  }
}

// ---- dense route (n_fft that fft_lds.h has no plan for, or DeviceFeatureExtractor(fft=False)): frames split for the bf16x3 STFT GEMM, then |.| + mel + log ----------
__device__ __forceinline__ void store_split4(uint16_t* dst, long seg, const float v[4]) {
  uint2 hi, lo;
  split_bf16x4(v[0], v[1], v[2], v[3], hi, lo);
  *reinterpret_cast<uint2*>(dst) = hi;
  *reinterpret_cast<uint2*>(dst + seg) = lo;
  *reinterpret_cast<uint2*>(dst + 2 * seg) = hi;
}
// As[row][3][n_fft]: the reflect-padded analysis frame of packed row `row` as [hi | lo | hi] (the window lives in the basis)
__global__ __launch_bounds__(256) void feat_frame_split_kernel(const float* __restrict__ wave, const int* __restrict__ len,
                                                               const int* __restrict__ offs, uint16_t* __restrict__ As, int U,
                                                               int Lmax, int hop, int n_fft, long rows) {
  const int q = n_fft / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * q) return;
  const int j4 = (int)(i % q) * 4;
  const long row = i / q;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (row < offs[U]) {
    const int u = feat_find(offs, U, (int)row), t = (int)row - offs[u], L = len[u];
    const float* w = wave + (long)u * Lmax;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int j = t * hop + j4 + e - n_fft / 2;
      if (j < 0) j = -j;
      if (j >= L) j = 2 * (L - 1) - j;
      v[e] = w[j];
    }
  }
  store_split4(As + row * 3 * n_fft + j4, n_fft, v);
}

constexpr int FEAT_MAX_F = 2049;
// Y [rows][re(0..F) pad | im(0..F) pad] (halves Fp apart) -> out[row][b] = log(max(sum_k |Y_k| mel[b][k], eps))
__global__ __launch_bounds__(256) void feat_stft_mel_kernel(const float* __restrict__ Y, const float* __restrict__ mel,
                                                            const int* __restrict__ range, float* __restrict__ out, long rows,
                                                            int F, int Fp, int n_bins, float eps) {
  __shared__ float mg[FEAT_MAX_F];
  const int tid = threadIdx.x;
  const float log_eps = (float)log((double)eps);
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* y = Y + row * 2 * Fp;
    for (int k = tid; k < F; k += 256) {
      const float re = y[k], im = y[Fp + k];
      mg[k] = sqrtf(re * re + im * im);
    }
    __syncthreads();
    for (int b = tid; b < n_bins; b += 256) {
      const float* m = mel + (long)b * F;
      float acc = 0.f;
      for (int k = range[2 * b]; k < range[2 * b + 1]; ++k) acc += mg[k] * m[k];
      out[row * n_bins + b] = acc > eps ? logf(acc) : log_eps;
    }
    __syncthreads();
  }
}

// mom[u][0][c] = sum_t x[t][c], mom[u][1][c] = sum_t x[t][c]^2 over utterance u's rows: lane r of 256 / n_bins row lanes
// folds rows r, r + R, .. in index order (double accumulators), then the lanes are folded in order 0 .. R - 1
__global__ __launch_bounds__(256) void feat_moments_kernel(const float* __restrict__ x, const int* __restrict__ offs,
                                                           float* __restrict__ mom, int n_bins) {
  __shared__ double ls[2][256];
  const int u = blockIdx.x, tid = threadIdx.x, R = 256 / n_bins;
  const int r = tid / n_bins, c = tid - r * n_bins;
  const long r0 = offs[u], r1 = offs[u + 1];
  double s = 0.0, s2 = 0.0;
  if (r < R)
    for (long t = r0 + r; t < r1; t += R) {
      const double v = (double)x[t * n_bins + c];
      s += v;
      s2 += v * v;
    }
  ls[0][tid] = s;
  ls[1][tid] = s2;
  __syncthreads();
  if (tid < n_bins) {
    double a = 0.0, a2 = 0.0;
    for (int i = 0; i < R; ++i) {
      a += ls[0][i * n_bins + tid];
      a2 += ls[1][i * n_bins + tid];
    }
    mom[((long)u * 2) * n_bins + tid] = (float)a;
    mom[((long)u * 2 + 1) * n_bins + tid] = (float)a2;
  }
}

// out [U][Tmax][n_bins]: +0.0 in the rows T_u .. Tmax of every utterance (what _collate_frames pads with); with the BATCH
// epilogue above, which writes rows 0 .. T_u, every element of `out` is written exactly once
__global__ __launch_bounds__(256) void feat_pad_rows_kernel(const int* __restrict__ len, float* __restrict__ out, int U, int Tmax,
                                                            int size, int hop, int n_bins) {
  for (int u = blockIdx.y; u < U; u += gridDim.y) {
    const int T = min(feat_frames(len[u], true, size, hop), Tmax);
    float* o = out + (long)u * Tmax * n_bins;
    const long end = (long)Tmax * n_bins;
    for (long i = (long)T * n_bins + blockIdx.x * 256 + threadIdx.x; i < end; i += (long)gridDim.x * 256) o[i] = 0.f;
  }
}

// pcm[b][i] = round-half-even(clip(wave[b][i], -1, 1 - 2^-15) * 2^15) for i < len[b], 0 behind it.  The product by 2^15 is
// exact in fp32, so these are the integers generate_waveform.write_wav forms in float64.
__global__ __launch_bounds__(256) void wave_to_pcm16_kernel(const float* __restrict__ wave, const int* __restrict__ len,
                                                            int16_t* __restrict__ pcm, int B, int N) {
  const int b = blockIdx.y;
  const int L = min(len[b], N);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
    const long at = (long)b * N + i;
    float v = 0.f;
    if (i < L) v = rintf(fminf(fmaxf(wave[at], -1.f), 1.f - 1.f / 32768.f) * 32768.f);
    pcm[at] = (int16_t)(int)v;
  }
}

template <int N, bool KALDI, bool BATCH = false>
int feat_fft_launch(const float* wave, const int* len, const float* win, const float* tw, const float* mel, const int* range,
                    float* out, int* offs, int U, int Lmax, int size, int hop, int n_bins, float eps, long n_pairs, long out_rows,
                    hipStream_t st, const float* cmean = nullptr, const float* cstd = nullptr, int Tmax = 0) {
  S2ST_LAUNCH(feat_offsets_kernel, dim3(1), dim3(256), 0, st, len, offs, U, KALDI ? 1 : 0, KALDI ? size : N, hop);
  if (n_pairs > 0) {
    // (a workgroup keeps its twiddle table and window over the pairs it walks: 8 workgroups per CU at most)
    const unsigned grid = (unsigned)(n_pairs < 2048 ? n_pairs : 2048);
    S2ST_LAUNCH((feat_fft_kernel<N, KALDI, BATCH>), dim3(grid), dim3(256), 0, st, wave, len, win,
                reinterpret_cast<const cplx*>(tw), mel, range, out, offs, U, Lmax, size, hop, n_bins, eps, out_rows, cmean, cstd,
                Tmax);
  }
  if (BATCH) {
    const long per = (long)Tmax * n_bins;
    S2ST_LAUNCH(feat_pad_rows_kernel, dim3((unsigned)(per < 64 * 256 ? (per + 255) / 256 : 64), (unsigned)(U < 1024 ? U : 1024)),
                dim3(256), 0, st, len, out, U, Tmax, size, hop, n_bins);
  }
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

}  // namespace

int s2st_fbank_kaldi(const float* wave, const int* len, const float* win, const float* tw, const float* banks, const int* range,
                     float* out, int* offs, int U, int Lmax, int size, int shift, int padded, int n_bins, float eps, long n_pairs,
                     long out_rows, hipStream_t st) {
  if (U <= 0) return 0;
  if (size < 2 || size > padded || shift < 1 || n_bins < 1 || Lmax < 1) return S2ST_ERR_SHAPE;
#define S2ST_FFT_CASE(N) \
  case N: return feat_fft_launch<N, true>(wave, len, win, tw, banks, range, out, offs, U, Lmax, size, shift, n_bins, eps, n_pairs, out_rows, st);
  switch (padded) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) }  // (Kaldi pads its frames to a power of two)
#undef S2ST_FFT_CASE
  return S2ST_ERR_SHAPE;
}

int s2st_fbank_kaldi_batch(const float* wave, const int* len, const float* win, const float* tw, const float* banks,
                           const int* range, const float* mean, const float* std, float* batch, int* offs, int U, int Lmax, int Tmax,
                           int size, int shift, int padded, int n_bins, float eps, long n_pairs, hipStream_t st) {
  if (U <= 0 || Tmax == 0) return 0;
  if (size < 2 || size > padded || shift < 1 || n_bins < 1 || Lmax < 1 || Tmax < 0) return S2ST_ERR_SHAPE;
#define S2ST_FFT_CASE(N) \
  case N: return feat_fft_launch<N, true, true>(wave, len, win, tw, banks, range, batch, offs, U, Lmax, size, shift, n_bins, eps, n_pairs, 0, st, mean, std, Tmax);
  switch (padded) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) }
#undef S2ST_FFT_CASE
  return S2ST_ERR_SHAPE;
}

int s2st_logmel(const float* wave, const int* len, const float* win, const float* tw, const float* mel, const int* range,
                float* out, int* offs, int U, int Lmax, int n_fft, int hop, int n_mels, float eps, long n_pairs, long out_rows,
                hipStream_t st) {
  if (U <= 0) return 0;
  if (hop < 1 || n_mels < 1 || Lmax < 1) return S2ST_ERR_SHAPE;
#define S2ST_FFT_CASE(N) \
  case N: return feat_fft_launch<N, false>(wave, len, win, tw, mel, range, out, offs, U, Lmax, n_fft, hop, n_mels, eps, n_pairs, out_rows, st);
  switch (n_fft) { S2ST_FFT_POW2_SIZES(S2ST_FFT_CASE) S2ST_FFT_MIXED_SIZES(S2ST_FFT_CASE) }
#undef S2ST_FFT_CASE
  return S2ST_ERR_SHAPE;
}

int s2st_logmel_frame_split(const float* wave, const int* len, uint16_t* As, int* offs, int U, int Lmax, int n_fft, int hop,
                            long rows, hipStream_t st) {
  if (U <= 0) return 0;
  if (n_fft % 4 || n_fft < 4 || hop < 1 || Lmax < 1) return S2ST_ERR_SHAPE;
  S2ST_LAUNCH(feat_offsets_kernel, dim3(1), dim3(256), 0, st, len, offs, U, 0, n_fft, hop);
  const long n = rows * (n_fft / 4);
  if (n > 0)
    S2ST_LAUNCH(feat_frame_split_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, wave, len, offs, As, U, Lmax, hop,
                n_fft, rows);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_logmel_from_stft(const float* Y, const float* mel, const int* range, float* out, long rows, int F, int Fp, int n_mels,
                          float eps, hipStream_t st) {
  if (rows <= 0) return 0;
  if (F < 1 || F > FEAT_MAX_F || Fp < F || n_mels < 1) return S2ST_ERR_SHAPE;
  S2ST_LAUNCH(feat_stft_mel_kernel, dim3((unsigned)(rows < 4096 ? rows : 4096)), dim3(256), 0, st, Y, mel, range, out, rows, F, Fp,
              n_mels, eps);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_feature_moments(const float* feats, const int* offs, float* mom, int U, int n_bins, hipStream_t st) {
  if (U <= 0) return 0;
  if (n_bins < 1 || n_bins > 256) return S2ST_ERR_SHAPE;
  S2ST_LAUNCH(feat_moments_kernel, dim3(U), dim3(256), 0, st, feats, offs, mom, n_bins);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_wave_pcm16(const float* wave, const int* len, int16_t* pcm, int B, int N, hipStream_t st) {
  if (B <= 0 || N == 0) return 0;
  if (N < 0 || B > 65535) return S2ST_ERR_SHAPE;
  S2ST_LAUNCH(wave_to_pcm16_kernel, dim3((unsigned)(N < 1024 * 256 ? (N + 255) / 256 : 1024), (unsigned)B), dim3(256), 0, st, wave,
              len, pcm, B, N);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
