// Kernels of the wav2vec 2.0 CTC recogniser (ASR-BLEU scoring of generated speech) that are not GEMMs, and the
// polyphase resampler in front of it.  Activations are channel-last [B][T][C].
//
// Reference call sites replaced (examples/s2s_trans/evalute_s2s_bleu.py: librosa.load(path, sr=16000),
// Wav2Vec2Processor(...), Wav2Vec2ForCTC(...).logits, torch.argmax(logits, dim=-1), processor.batch_decode):
//   * transformers Wav2Vec2FeatureExtractor.zero_mean_unit_var_norm (per utterance over its valid samples),
//   * Wav2Vec2LayerNormConvLayer (Conv1d + bias -> LayerNorm over channels -> GELU), first layer fused with its convolution,
//     later layers as a row kernel behind the conv-as-GEMM,
//   * argmax + Wav2Vec2CTCTokenizer's collapse (repeats merged, pad dropped) over the valid frames,
//   * resampy's kaiser_best band-limited interpolation (what librosa.load's resampling evaluates), as a polyphase table.
// No atomics anywhere: every reduction has a fixed order, results repeat bit for bit.
#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

// sum over the workgroup's 256 threads in a fixed tree order (every thread gets the result)
__device__ __forceinline__ double block_sum256(double v, double* sm) {
  const int tid = threadIdx.x;
  __syncthreads();  // (sm may still be read from the previous reduction)
  sm[tid] = v;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) sm[tid] += sm[tid + s];
    __syncthreads();
  }
  return sm[0];
}

// y[b][i] = (x[b][i] - mean_b) / sqrt(var_b + eps) for i < n_b, 0 behind (the processor pads AFTER normalising);
// mean / biased variance over the n_b valid samples, two passes, float64 partial sums: thread t adds samples t, t + 256, ..
// in order, then the tree above -- one order whatever else is in the batch.  One workgroup per utterance.
__global__ __launch_bounds__(256) void wave_norm_kernel(const float* __restrict__ x, const int* __restrict__ lens,
                                                        float* __restrict__ y, int N, float eps) {
  __shared__ double sm[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), N);
  const float* xb = x + (long)b * N;
  float* yb = y + (long)b * N;
  double s = 0.0;
  for (int i = tid; i < n; i += 256) s += (double)xb[i];
  const double mean = n > 0 ? block_sum256(s, sm) / n : 0.0;
  double q = 0.0;
  for (int i = tid; i < n; i += 256) {
    const double d = (double)xb[i] - mean;
    q += d * d;
  }
  const double var = n > 0 ? block_sum256(q, sm) / n : 0.0;
  const float mu = (float)mean, rs = (float)(1.0 / sqrt(var + (double)eps));
  for (int i = tid; i < N; i += 256) yb[i] = i < n ? (xb[i] - mu) * rs : 0.f;
}

// First block of the "layer-norm" feature extractor, fused: per frame conv0[c] = bias[c] + sum_j w[c][j] x[t stride + j],
// LayerNorm over the C channels (two passes over registers), GELU.  A WAVE owns a frame: lane l holds channels l, l + 64, ..
// (CPL of them: 8 for C = 512), so a frame's statistics are two wave reductions and its stores are 256-byte rows; the frame's
// samples sit at wave-uniform addresses.  A workgroup (4 waves) owns CL_FT consecutive frames of one utterance.
// The output is the largest tensor of the forward: fast mode stores only the bf16 copy the next convolution's GEMM reads.
constexpr int CL_FT = 64, CL_MAXK = 16;
template <int CPL, int KT>
__global__ __launch_bounds__(256) void conv0_ln_gelu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            uint16_t* __restrict__ yh, int N, int T, int C, int k, int stride,
                                                            float eps) {
  constexpr bool GEN = KT == CL_MAXK;
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int t0 = blockIdx.x * CL_FT + wv * (CL_FT / 4), t1 = min(t0 + CL_FT / 4, T);
  const float* xu = x + (long)b * N;
  float wr[CPL][KT], bs[CPL], ga[CPL], be[CPL];
#pragma unroll
  for (int e = 0; e < CPL; ++e) {
    const int c = lane + 64 * e;
    const bool ok = c < C;
    bs[e] = ok ? bias[c] : 0.f;
    ga[e] = ok ? gamma[c] : 0.f;
    be[e] = ok ? beta[c] : 0.f;
#pragma unroll
    for (int j = 0; j < KT; ++j) wr[e][j] = (ok && (!GEN || j < k)) ? w[(long)c * k + j] : 0.f;
  }
  const float invC = 1.f / (float)C;
  for (int t = t0; t < t1; ++t) {
    const float* xf = xu + (long)t * stride;  // (wave-uniform: the frame's samples are scalar loads)
    float xv[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) xv[j] = xf[GEN ? min(j, k - 1) : j];
    float a[CPL];
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
      float v = bs[e];
#pragma unroll
      for (int j = 0; j < KT; ++j) v = fmaf(wr[e][j], xv[j], v);
      a[e] = v;
      s += (lane + 64 * e < C) ? v : 0.f;
    }
    const float mean = wave_sum(s) * invC;
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
      const float d = (lane + 64 * e < C) ? a[e] - mean : 0.f;
      q = fmaf(d, d, q);
    }
    const float rstd = rsqrtf(wave_sum(q) * invC + eps);
    const long o = ((long)b * T + t) * C;
#pragma unroll
    for (int e = 0; e < CPL; ++e) {
      const int c = lane + 64 * e;
      if (c < C) {
        const float v = gelu_erf((a[e] - mean) * rstd * ga[e] + be[e]);
        if (y) y[o + c] = v;
        if (yh) yh[o + c] = (uint16_t)(pack_bf16x4(v, 0.f, 0.f, 0.f).x & 0xffffu);
      }
    }
  }
}

// y[r][:] = gelu(LayerNorm(x[r][:]) * gamma + beta): the conv layers behind the first (the GEMM's epilogue added the bias;
// GELU comes AFTER the norm here, so the GEMM's own GELU epilogue cannot be used).  One wave per row, the row in registers
// (C <= 256 * LG_MAXE, C % 4 == 0); writes the fp32 copy, the bf16 operand copy, or both; y == x (in place) is allowed.
constexpr int LG_MAXE = 4;
__global__ __launch_bounds__(256) void ln_gelu_rows_kernel(const float* x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* y, uint16_t* __restrict__ yh,
                                                           int rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;  // (whole waves leave: no collective below is split)
  const float* xr = x + (long)r * C;
  float4 v[LG_MAXE];
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < LG_MAXE; ++e) {
    const int c = lane * 4 + 256 * e;
    v[e] = c < C ? *reinterpret_cast<const float4*>(xr + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    s += (v[e].x + v[e].y) + (v[e].z + v[e].w);
  }
  const float invC = 1.f / (float)C;
  const float mean = wave_sum(s) * invC;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < LG_MAXE; ++e) {
    if (lane * 4 + 256 * e < C) {
      const float d0 = v[e].x - mean, d1 = v[e].y - mean, d2 = v[e].z - mean, d3 = v[e].w - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  const float rstd = rsqrtf(wave_sum(q) * invC + eps);
#pragma unroll
  for (int e = 0; e < LG_MAXE; ++e) {
    const int c = lane * 4 + 256 * e;
    if (c < C) {
      const float4 g = *reinterpret_cast<const float4*>(gamma + c), bb = *reinterpret_cast<const float4*>(beta + c);
      const float o0 = gelu_erf((v[e].x - mean) * rstd * g.x + bb.x), o1 = gelu_erf((v[e].y - mean) * rstd * g.y + bb.y);
      const float o2 = gelu_erf((v[e].z - mean) * rstd * g.z + bb.z), o3 = gelu_erf((v[e].w - mean) * rstd * g.w + bb.w);
      if (y) *reinterpret_cast<float4*>(y + (long)r * C + c) = make_float4(o0, o1, o2, o3);
      if (yh) *reinterpret_cast<uint2*>(yh + (long)r * C + c) = pack_bf16x4(o0, o1, o2, o3);
    }
  }
}

// Greedy CTC decoding of one utterance per workgroup: frame t < len keeps its argmax a_t (ties to the lowest id, as
// torch.argmax) iff a_t != blank and a_t != a_(t-1); the survivors are compacted in frame order with a wave prefix count
// (ballot + popcount below the lane) and a running base across waves and 256-frame chunks.  ids[b][0 .. count) = the kept
// ids, -1 behind; counts[b] = count.  Frames at or past len are never read.
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ logits, const int* __restrict__ lens,
                                                         int* __restrict__ ids, int* __restrict__ counts, int T, int V,
                                                         int blank) {
  __shared__ int s_arg[257];
  __shared__ int s_wave[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int len = min(max(lens[b], 0), T);
  const float* lg = logits + (long)b * T * V;
  int* out = ids + (long)b * T;
  int base = 0;
  if (tid == 0) s_arg[0] = -1;  // (no frame in front of frame 0)
  for (int c0 = 0; c0 < len; c0 += 256) {
    const int t = c0 + tid;
    int am = -1;
    if (t < len) {
      const float* row = lg + (long)t * V;
      float best = row[0];
      am = 0;
      for (int v = 1; v < V; ++v) {
        const float z = row[v];
        if (z > best) { best = z; am = v; }
      }
    }
    __syncthreads();  // (the previous chunk's readers of s_arg are done; s_arg[0] holds its last frame)
    s_arg[tid + 1] = am;
    __syncthreads();
    const int keep = (t < len && am != blank && am != s_arg[tid]) ? 1 : 0;
    const unsigned long long m = __ballot(keep);
    const int below = __builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wv] = __builtin_popcountll(m);
    __syncthreads();
    int off = base;
    for (int i = 0; i < wv; ++i) off += s_wave[i];
    if (keep) out[off + below] = am;
    base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const int last = s_arg[256];
    __syncthreads();
    if (tid == 0) s_arg[0] = last;
  }
  for (int i = base + tid; i < T; i += 256) out[i] = -1;
  if (tid == 0) counts[b] = base;
}

// Polyphase band-limited resampling by the rational factor L / M (output sample t sits at input time t M / L): phase
// p = (t M) mod L, n = (t M) div L, y[t] = sum_d table[p][d] x[n - KL + 1 + d], d = 0 .. KW - 1, samples outside [0, n_in)
// read as 0 (the filter's wings stop at the signal's ends).  The table holds the interpolated filter values of every phase
// (computed once on the host in float64); the taps are added in table order.  y[b][t] = 0 for t >= ceil(n_in L / M).
__global__ __launch_bounds__(256) void resample_sinc_kernel(const float* __restrict__ x, const int* __restrict__ n_in,
                                                            const float* __restrict__ table, float* __restrict__ y, int N_in,
                                                            int N_out, int L, int M, int KL, int KW) {
  const int b = blockIdx.y;
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= N_out) return;
  const int ni = min(max(n_in[b], 0), N_in);
  const long no = ((long)ni * L + M - 1) / M;
  float acc = 0.f;
  if (t < no) {
    const long tm = t * M;
    const int p = (int)(tm % L);
    const long n = tm / L;
    const float* tp = table + (long)p * KW;
    const float* xb = x + (long)b * N_in;
    const long i0 = n - KL + 1;
    const int d0 = (int)max(0L, -i0), d1 = (int)min((long)KW, (long)ni - i0);
    for (int d = d0; d < d1; ++d) acc = fmaf(tp[d], xb[i0 + d], acc);
  }
  y[(long)b * N_out + t] = acc;
}

}  // namespace

int s2st_w2v_wave_norm(const float* x, const int* lens, float* y, int B, int N, float eps, hipStream_t st) {
  if (B <= 0 || N <= 0) return 0;
  S2ST_LAUNCH(wave_norm_kernel, dim3(B), dim3(256), 0, st, x, lens, y, N, eps);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_w2v_conv0_ln_gelu(const float* x, const float* w, const float* bias, const float* gamma, const float* beta, float* y,
                           uint16_t* yh, int B, int N, int T, int C, int k, int stride, float eps, hipStream_t st) {
  if (C < 1 || C > 512 || k < 1 || k > CL_MAXK || stride < 1) return S2ST_ERR_SHAPE;
  if (B <= 0 || T <= 0) return 0;
  if ((long)(T - 1) * stride + k > N) return S2ST_ERR_SHAPE;  // (every frame's window lies inside the row)
  const dim3 grid((T + CL_FT - 1) / CL_FT, B);
#define S2ST_CL_LAUNCH(CPL, KT) \
  S2ST_LAUNCH((conv0_ln_gelu_kernel<CPL, KT>), grid, dim3(256), 0, st, x, w, bias, gamma, beta, y, yh, N, T, C, k, stride, eps)
  if (C <= 64) {
    if (k == 10) S2ST_CL_LAUNCH(1, 10); else S2ST_CL_LAUNCH(1, CL_MAXK);
  } else {
    if (k == 10) S2ST_CL_LAUNCH(8, 10); else S2ST_CL_LAUNCH(8, CL_MAXK);
  }
#undef S2ST_CL_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_w2v_ln_gelu_rows(const float* x, const float* gamma, const float* beta, float* y, uint16_t* yh, int rows, int C,
                          float eps, hipStream_t st) {
  if (C < 4 || C % 4 || C > 256 * LG_MAXE) return S2ST_ERR_SHAPE;
  if (rows <= 0) return 0;
  S2ST_LAUNCH(ln_gelu_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, x, gamma, beta, y, yh, rows, C, eps);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_w2v_ctc_greedy(const float* logits, const int* lens, int* ids, int* counts, int B, int T, int V, int blank,
                        hipStream_t st) {
  if (V < 1) return S2ST_ERR_SHAPE;
  if (B <= 0 || T <= 0) return 0;
  S2ST_LAUNCH(ctc_greedy_kernel, dim3(B), dim3(256), 0, st, logits, lens, ids, counts, T, V, blank);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_resample_sinc(const float* x, const int* n_in, const float* table, float* y, int B, int N_in, int N_out, int L, int M,
                       int KL, int KW, hipStream_t st) {
  if (L < 1 || M < 1 || KW < 1 || KL < 1 || KL > KW) return S2ST_ERR_SHAPE;
  if (B <= 0 || N_out <= 0 || N_in <= 0) return 0;
  if (B > 65535) return S2ST_ERR_SHAPE;
  S2ST_LAUNCH(resample_sinc_kernel, dim3((N_out + 255) / 256, B), dim3(256), 0, st, x, n_in, table, y, N_in, N_out, L, M, KL,
              KW);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
