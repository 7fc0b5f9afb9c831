// Inference-only kernels of the AR mel decoder (config 5).
//
// Reference call sites replaced: fairseq/modules/multihead_attention.py:194-385 with
// incremental_state (one query per utterance against the cached keys / values, key padding mask,
// head-averaged weights of the alignment layer) and fairseq/speech_generator_for_s2st.py:88-110
// (sigmoid of the stop logits, argmax alignment, global-CMVN de-normalisation).
#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

constexpr int DA_MAXS = 4096;

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// one query per (b, h): o[b][h*dh + d] = sum_s softmax_s(scale q.k_s) v_s[d]; optional
// attn_mean[b][s] += p_s / H (zero-initialised by the launcher)
// k_new / v_new (self-attention of a decoding step): the step's key / value rows [B][ld_new]; the workgroup first stores its
// (b, h) slice as row pos_new of the caches (no other workgroup reads or writes that slice), then attends over the cache
__global__ __launch_bounds__(256) void decode_attn_kernel(const float* __restrict__ q, long ldq,
                                                          float* __restrict__ kc, float* __restrict__ vc,
                                                          long ldk, long kbs, const int* __restrict__ klen, int nkeys,
                                                          int H, int dh, float scale, float* __restrict__ o, long ldo,
                                                          float* __restrict__ attn_mean, int S,
                                                          const float* __restrict__ k_new, const float* __restrict__ v_new,
                                                          long ld_new, int pos_new, const int* __restrict__ step_ptr) {
  if (step_ptr) { pos_new = *step_ptr; nkeys = pos_new + 1; }  // (replayable step: the step lives in device memory)
  __shared__ float p[DA_MAXS];
  __shared__ __attribute__((aligned(16))) float qs[256];
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) float part[16 * 256];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, tid = threadIdx.x;
  const int n = klen ? min((int)klen[b], nkeys) : nkeys;
  if (tid < dh) qs[tid] = q[(long)b * ldq + h * dh + tid] * scale;
  if (k_new && tid < dh) {
    kc[(long)b * kbs + (long)pos_new * ldk + h * dh + tid] = k_new[(long)b * ld_new + h * dh + tid];
    vc[(long)b * kbs + (long)pos_new * ldk + h * dh + tid] = v_new[(long)b * ld_new + h * dh + tid];
  }
  __syncthreads();  // (workgroup-scope: the stores above are visible to this workgroup's loads below)
  const float* kb = kc + (long)b * kbs + h * dh;
  const float* vb = vc + (long)b * kbs + h * dh;
  // 16 lanes per key, one float4 each: a 64-wide head row is one coalesced 256-byte read; 16 keys per pass
  const int g = tid >> 4, l4 = (tid & 15) * 4;
  // (4 keys per thread and pass, loads clamped instead of predicated so that they issue back to back:
  // the kernel is a chain of memory latencies otherwise)
  // (round 4: 8 keys per thread and pass -- 128 keys per workgroup and pass, every load of a pass issued before the first
  // multiply: the ~350 encoder positions of a cross-attention are 3 memory round trips instead of 6 x 2)
  constexpr int KP = 8;
  float mx = -INFINITY;
  if (dh <= 128 && dh % 64 == 0) {
    const int nd = dh / 64;  // 1 or 2 float4 chunks per lane
    for (int s0 = 0; s0 < n; s0 += 16 * KP) {
      float4 kv[2][KP];
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < KP; ++i)
          kv[c][i] = *reinterpret_cast<const float4*>(kb + (long)min(s0 + g + 16 * i, n - 1) * ldk + min(l4 + 64 * c, dh - 4));
      float a[KP];
#pragma unroll
      for (int i = 0; i < KP; ++i) a[i] = 0.f;
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (c >= nd) break;
        const float4 qv = *reinterpret_cast<const float4*>(qs + l4 + 64 * c);
#pragma unroll
        for (int i = 0; i < KP; ++i) a[i] += qv.x * kv[c][i].x + qv.y * kv[c][i].y + qv.z * kv[c][i].z + qv.w * kv[c][i].w;
      }
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        float v = a[i];
        v += __shfl_xor(v, 8);
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 2);
        v += __shfl_xor(v, 1);
        const int s = s0 + g + 16 * i;
        if (s < n) {
          if (l4 == 0) p[s] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
  } else
  for (int s0 = 0; s0 < n; s0 += 64) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = l4; d < dh; d += 64) {
      float4 kv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) kv[i] = *reinterpret_cast<const float4*>(kb + (long)min(s0 + g + 16 * i, n - 1) * ldk + d);
      const float4 qv = *reinterpret_cast<const float4*>(qs + d);
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] += qv.x * kv[i].x + qv.y * kv[i].y + qv.z * kv[i].z + qv.w * kv[i].w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = a[i];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 1);
      const int s = s0 + g + 16 * i;
      if (s < n) {
        if (l4 == 0) p[s] = v;
        mx = fmaxf(mx, v);
      }
    }
  }
  mx = block_max(mx, red);
  float sum = 0.f;
  for (int s = tid; s < n; s += 256) {
    const float e = __expf(p[s] - mx);
    p[s] = e;
    sum += e;
  }
  sum = block_sum(sum, red);
  const float inv = sum > 0.f ? 1.f / sum : 0.f;
  __syncthreads();
  // o: 16 key slices x (16 lanes x float4) per 64 head columns, slices combined in a fixed order
  for (int d = l4; d < dh; d += 64) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < n; s0 += 16 * KP) {  // (8 value rows per thread in flight; same accumulation order as before)
      float4 vv[KP];
      float w[KP];
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        const int s = s0 + g + 16 * i;
        vv[i] = *reinterpret_cast<const float4*>(vb + (long)min(s, n - 1) * ldk + d);
        w[i] = s < n ? p[s] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        acc.x += w[i] * vv[i].x; acc.y += w[i] * vv[i].y; acc.z += w[i] * vv[i].z; acc.w += w[i] * vv[i].w;
      }
    }
    *reinterpret_cast<float4*>(part + g * dh + d) = acc;
  }
  __syncthreads();
  if (tid < dh) {
    float a = 0.f;
    for (int i = 0; i < 16; ++i) a += part[i * dh + tid];
    o[(long)b * ldo + h * dh + tid] = a * inv;
  }
  if (attn_mean)
    for (int s = tid; s < n; s += 256) atomicAdd(attn_mean + (long)b * S + s, p[s] * inv / H);
}

__global__ __launch_bounds__(256) void sigmoid_kernel(const float* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = 1.f / (1.f + __expf(-x[i]));
}

// x [B][E][D] -> idx[b][d] = first argmax_e x[b][e][d]
__global__ __launch_bounds__(256) void argmax_dim1_kernel(const float* __restrict__ x, long* __restrict__ idx, int B,
                                                          int E, int D) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)B * D) return;
  const int b = (int)(i / D), d = (int)(i - (long)b * D);
  const float* xb = x + (long)b * E * D + d;
  float best = xb[0];
  int bi = 0;
  for (int e = 1; e < E; ++e) {
    const float v = xb[(long)e * D];
    if (v > best) { best = v; bi = e; }
  }
  idx[i] = bi;
}

// y[r][c] = x[r][c] * scale[c] + shift[c]
__global__ __launch_bounds__(256) void affine_cols_kernel(const float* __restrict__ x, const float* __restrict__ sc,
                                                          const float* __restrict__ sh, float* __restrict__ y,
                                                          long rows, int C) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * C) return;
  const int c = (int)(i % C);
  y[i] = x[i] * sc[c] + sh[c];
}

// The same attention for head widths 64 / 128 (round 4, second form).  The kernel above is a chain of memory round trips:
// key lengths and the query (-> LDS, barrier), key passes, two block-wide reductions, then value passes (x 2 column halves
// at width 128): 5.3 us for ONE key, 18 us for 315, and a batch's launch lasts as long as its longest utterance's
// workgroup (tools/decode_attn_bench.py, profiles/r04_t_decode_attn_bench.txt).  Here
//   * every 16-lane group keeps a RUNNING softmax over its own keys (s = g mod G): keys AND values of a pass are loaded
//     together, scores -> running maximum -> rescale -> accumulate; the G groups are merged once at the end through LDS in
//     group order (no block-wide reduction inside the loop, no atomics);
//   * the first pass's loads wait for the utterance's key count only: the query comes straight from global memory, and the
//     step's own key / value row is taken from k_new / v_new in registers (and stored to the cache for the later steps)
//     instead of being stored, fenced by a barrier and read back.  (Clamping the rows to the cache's extent instead of
//     the utterance's length, so that not even the key count is waited for, was tried: every workgroup then fetches a full
//     pass of distinct rows -- 67 MB per launch instead of 23 MB for the bench batch -- and the launch takes 20 us);
//   * NT = 1024 threads (64 groups: 256 keys per pass in fp32, 512 with bf16 rows) and KT = bf16raw (the static
//     cross-attention rows as bf16) are built and tested but NOT the default: measured on the bench batch (64 utterances x 4
//     heads of width 128, 8 - 315 keys, tools/decode_attn_bench.py) 16.3 us and 13.9 us against 13.3 us for 256 threads on
//     fp32 rows -- a launch lasts as long as its longest utterance's workgroup, which pulls its rows at ~20 B/clk whatever
//     their type, and the wider forms start later (5.8 us for one key with 256 threads on fp32, 8.4 with bf16, 9.3 with
//     1024 threads).
template <typename KT>
struct RawRow;
template <>
struct RawRow<float> {
  typedef float4 T;
  static __device__ __forceinline__ float4 cvt(const float4& r) { return r; }
};
template <>
struct RawRow<bf16raw> {
  typedef uint2 T;
  static __device__ __forceinline__ float4 cvt(const uint2& u) {
    return float4{__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                  __uint_as_float(u.y & 0xffff0000u)};
  }
};

template <typename KT, int ND, int NT>
__global__ __launch_bounds__(NT) void decode_attn_fast_kernel(const float* __restrict__ q, long ldq, KT* __restrict__ kc,
                                                              KT* __restrict__ vc, long ldk, long kbs,
                                                              const int* __restrict__ klen, int nkeys, int H, float scale,
                                                              float* __restrict__ o, long ldo, float* __restrict__ attn_mean,
                                                              int S, const float* __restrict__ k_new,
                                                              const float* __restrict__ v_new, long ld_new, int pos_new,
                                                              const int* __restrict__ step_ptr) {
  if (step_ptr) { pos_new = *step_ptr; nkeys = pos_new + 1; }  // (replayable step: the step lives in device memory)
  constexpr int dh = 64 * ND, G = NT / 16;
  constexpr int KP = (sizeof(KT) == 2 ? 16 : 8) / (NT / 256 > 2 ? 2 : 1);
  typedef typename RawRow<KT>::T Raw;
  __shared__ float p[DA_MAXS];
  __shared__ float gm[G], gl[G];
  __shared__ __attribute__((aligned(16))) float part[G * dh];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, tid = threadIdx.x;
  const int g = tid >> 4, l4 = (tid & 15) * 4;
  const KT* kb = kc + (long)b * kbs + h * dh;
  const KT* vb = vc + (long)b * kbs + h * dh;
  const int row_new = (sizeof(KT) == 4 && k_new) ? pos_new : -1;
  // ---- everything below up to the first use is independent loads ----
  const int n = klen ? min((int)klen[b], nkeys) : nkeys;
  float4 qv[ND], kn[ND], vn[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c) {
    qv[c] = *reinterpret_cast<const float4*>(q + (long)b * ldq + h * dh + l4 + 64 * c);
    if (row_new >= 0) {
      kn[c] = *reinterpret_cast<const float4*>(k_new + (long)b * ld_new + h * dh + l4 + 64 * c);
      vn[c] = *reinterpret_cast<const float4*>(v_new + (long)b * ld_new + h * dh + l4 + 64 * c);
    } else {
      kn[c] = vn[c] = float4{0.f, 0.f, 0.f, 0.f};
    }
  }
  float m_run = -INFINITY, l_run = 0.f;
  float4 acc[ND];
#pragma unroll
  for (int c = 0; c < ND; ++c) acc[c] = float4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = 0; s0 < n; s0 += G * KP) {
    Raw kr[ND][KP], vr[ND][KP];
#pragma unroll
    for (int c = 0; c < ND; ++c)
#pragma unroll
      for (int i = 0; i < KP; ++i)
        kr[c][i] = *reinterpret_cast<const Raw*>(kb + (long)min(s0 + g + G * i, n - 1) * ldk + l4 + 64 * c);
#pragma unroll
    for (int c = 0; c < ND; ++c)
#pragma unroll
      for (int i = 0; i < KP; ++i)
        vr[c][i] = *reinterpret_cast<const Raw*>(vb + (long)min(s0 + g + G * i, n - 1) * ldk + l4 + 64 * c);
    if (s0 == 0) {
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        qv[c].x *= scale; qv[c].y *= scale; qv[c].z *= scale; qv[c].w *= scale;
      }
    }
    float a[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) a[i] = 0.f;
#pragma unroll
    for (int c = 0; c < ND; ++c)
#pragma unroll
      for (int i = 0; i < KP; ++i) {
        float4 k4 = RawRow<KT>::cvt(kr[c][i]);
        if (s0 + g + G * i == row_new) k4 = kn[c];
        a[i] += qv[c].x * k4.x + qv[c].y * k4.y + qv[c].z * k4.z + qv[c].w * k4.w;
      }
    float pm = -INFINITY;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      float v = a[i];
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 1);
      const int s = s0 + g + G * i;
      if (s < n) {
        if (attn_mean && l4 == 0) p[s] = v;
        pm = fmaxf(pm, v);
      } else {
        v = -INFINITY;
      }
      a[i] = v;
    }
    if (pm == -INFINITY) continue;  // (none of this group's keys of the pass exists)
    const float m_new = fmaxf(m_run, pm);
    const float sc = __expf(m_run - m_new);  // (first pass: exp(-inf) = 0)
    l_run *= sc;
#pragma unroll
    for (int c = 0; c < ND; ++c) {
      acc[c].x *= sc; acc[c].y *= sc; acc[c].z *= sc; acc[c].w *= sc;
    }
#pragma unroll
    for (int i = 0; i < KP; ++i) {
      const bool on = a[i] != -INFINITY;
      const float e = on ? __expf(a[i] - m_new) : 0.f;
      l_run += e;
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        float4 v4 = RawRow<KT>::cvt(vr[c][i]);
        if (s0 + g + G * i == row_new) v4 = vn[c];
        if (!on) v4 = float4{0.f, 0.f, 0.f, 0.f};  // (a row behind the utterance's end may hold anything)
        acc[c].x += e * v4.x; acc[c].y += e * v4.y; acc[c].z += e * v4.z; acc[c].w += e * v4.w;
      }
    }
    m_run = m_new;
  }
  if constexpr (sizeof(KT) == 4) {
    if (row_new >= 0 && g == 0) {  // this step's rows into the caches (read by the later steps' launches)
#pragma unroll
      for (int c = 0; c < ND; ++c) {
        *reinterpret_cast<float4*>(kc + (long)b * kbs + (long)row_new * ldk + h * dh + l4 + 64 * c) = kn[c];
        *reinterpret_cast<float4*>(vc + (long)b * kbs + (long)row_new * ldk + h * dh + l4 + 64 * c) = vn[c];
      }
    }
  }
  if (l4 == 0) {
    gm[g] = m_run;
    gl[g] = l_run;
  }
#pragma unroll
  for (int c = 0; c < ND; ++c) *reinterpret_cast<float4*>(part + g * dh + l4 + 64 * c) = acc[c];
  __syncthreads();
  // merge of the G groups, in group order
  float M = gm[0];
  for (int i = 1; i < G; ++i) M = fmaxf(M, gm[i]);
  float Lsum = 0.f;
  for (int i = 0; i < G; ++i) Lsum += gm[i] == -INFINITY ? 0.f : gl[i] * __expf(gm[i] - M);
  const float inv = Lsum > 0.f ? 1.f / Lsum : 0.f;
  if (tid < dh) {
    float a = 0.f;
    for (int i = 0; i < G; ++i) a += gm[i] == -INFINITY ? 0.f : part[i * dh + tid] * __expf(gm[i] - M);
    o[(long)b * ldo + h * dh + tid] = a * inv;
  }
  if (attn_mean)
    for (int s = tid; s < n; s += NT) atomicAdd(attn_mean + (long)b * S + s, __expf(p[s] - M) * inv / H);
}

}  // namespace

// fairseq's reorder_incremental_state for the cached keys / values of a beam search (sequence_generator.py:393-400,
// multihead_attention.py:387-403): dst[n][b][0 : valid) = src[n][idx[b]][0 : valid) for the nb (layer, K | V) arrays.
namespace {
__global__ __launch_bounds__(256) void cache_reorder_kernel(const float4* __restrict__ src, float4* __restrict__ dst,
                                                            const int* __restrict__ idx, int Bb, long row4, long valid4) {
  const int b = blockIdx.x, n = blockIdx.y;
  const float4* s = src + ((long)n * Bb + idx[b]) * row4;
  float4* d = dst + ((long)n * Bb + b) * row4;
  for (long i = threadIdx.x; i < valid4; i += 256) d[i] = s[i];
}
}  // namespace
int s2st_cache_reorder(const float* src, float* dst, const int* idx, int nb, int Bb, long row_floats, long valid_floats,
                       hipStream_t st) {
  if (nb <= 0 || Bb <= 0 || valid_floats <= 0) return 0;
  if (row_floats % 4 || valid_floats % 4 || ((uintptr_t)src % 16) || ((uintptr_t)dst % 16) || !idx) return S2ST_ERR_ARG;
  S2ST_LAUNCH(cache_reorder_kernel, dim3(Bb, nb), dim3(256), 0, st, reinterpret_cast<const float4*>(src),
              reinterpret_cast<float4*>(dst), idx, Bb, row_floats / 4, valid_floats / 4);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_decode_attn(const float* q, long ldq, float* kc, float* vc, long ldk, long kbs, const int* klen,
                     int nkeys, int B, int H, int dh, float scale, float* o, long ldo, float* attn_mean, int S,
                     hipStream_t st, const float* k_new, const float* v_new, long ld_new, int pos_new, int kv_bf16,
                     const int* step_ptr) {
  if (B <= 0) return 0;
  if (nkeys > DA_MAXS || dh > 256 || dh % 4 || 256 % dh) return S2ST_ERR_SHAPE;
  if ((k_new != nullptr) != (v_new != nullptr) || (k_new && !step_ptr && (pos_new < 0 || pos_new >= nkeys))) return S2ST_ERR_ARG;
  if (kv_bf16 && (k_new || (dh != 64 && dh != 128) || ldk % 4)) return S2ST_ERR_ARG;  // (bf16 caches: static rows only)
  if (nkeys < 1) return S2ST_ERR_ARG;
  if (attn_mean) hipMemsetAsync(attn_mean, 0, sizeof(float) * (size_t)B * S, st);
  // (round 4's A/B forms are closed and gone: the two-pass first kernel stays only as the fallback for head widths other
  //  than 64 / 128; 64 key groups per workgroup measured 16.3 against 13.3 us on the bench batch, profiles/r04_t_decode_attn_bench.txt)
  const bool fast_ok = (dh == 64 || dh == 128) && ldk % 4 == 0 && ldq % 4 == 0 && (!k_new || ld_new % 4 == 0);
  if (kv_bf16 && !fast_ok) return S2ST_ERR_ARG;
#define S2ST_DA_LAUNCH(KT_, ND_, NT_, kp, vp)                                                                               \
  S2ST_LAUNCH((decode_attn_fast_kernel<KT_, ND_, NT_>), dim3(B * H), dim3(NT_), 0, st, q, ldq, kp, vp, ldk, kbs, klen, nkeys, H, \
              scale, o, ldo, attn_mean, S, k_new, v_new, ld_new, pos_new, step_ptr)
  if (!fast_ok) {
    S2ST_LAUNCH(decode_attn_kernel, dim3(B * H), dim3(256), 0, st, q, ldq, kc, vc, ldk, kbs, klen, nkeys, H, dh,
                scale, o, ldo, attn_mean, S, k_new, v_new, ld_new, pos_new, step_ptr);
  } else if (kv_bf16) {
    bf16raw* kh = reinterpret_cast<bf16raw*>(kc);
    bf16raw* vh = reinterpret_cast<bf16raw*>(vc);
    if (dh == 64) S2ST_DA_LAUNCH(bf16raw, 1, 256, kh, vh);
    else S2ST_DA_LAUNCH(bf16raw, 2, 256, kh, vh);
  } else {
    if (dh == 64) S2ST_DA_LAUNCH(float, 1, 256, kc, vc);
    else S2ST_DA_LAUNCH(float, 2, 256, kc, vc);
  }
#undef S2ST_DA_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

namespace {
__global__ __launch_bounds__(256) void scale_rows_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                         float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) y[i] = a[0] * x[i];
}
}  // namespace

// y = a[0] * x (a: one device scalar): the alpha-scaled position table of a decoding run
int s2st_scale_rows(const float* x, const float* a, float* y, long n, hipStream_t st) {
  if (n <= 0) return 0;
  S2ST_LAUNCH(scale_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, a, y, n);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

namespace {
// The generator's stop rule on the device (speech_generator_for_s2st.py:88-99), one workgroup: after step `step`
//   cur_finished = eos_prob > thr ; out_lens[~finished & cur_finished] = step + 1 ; finished |= cur_finished
// and the key lengths of the NEXT step's self-attention, cur_out_lens of :84-85 (out_lens with the "still running" value
// max_iter replaced by step + 2).  n_done[step] = number of finished utterances after this step: the host reads it a few
// steps late (no synchronisation inside the loop) and discards the steps it ran past the stop.
__global__ __launch_bounds__(256) void decode_stop_update_kernel(const float* __restrict__ eos_prob, float thr, int step,
                                                                 int max_iter, int B, int* __restrict__ finished,
                                                                 int* __restrict__ out_lens, int* __restrict__ klen_next,
                                                                 int* __restrict__ n_done) {
  __shared__ int cnt[4];
  int c = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const int cur = eos_prob[b] > thr ? 1 : 0;
    int f = finished[b], ol = out_lens[b];
    if (!f && cur) ol = step + 1;
    f |= cur;
    finished[b] = f;
    out_lens[b] = ol;
    klen_next[b] = ol == max_iter ? step + 2 : ol;
    c += f;
  }
  c = (int)wave_sum((float)c);
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) n_done[step] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
}

// ---- replayable decode step (engine.cpp, include/s2st_hip.h s2st_decode_replay) ---------------------------------------
// Seeds as the host derives them: decode_step gets seed0 + step, its i-th dropout site next_seed() = seed * 0x100000001B3 +
// (i + 1) * 0x9E3779B97F4A7C15 (engine.cpp next_seed; site counts from 1).
__device__ __forceinline__ uint64_t replay_site_seed(uint64_t seed0, int step, int site) {
  return (seed0 + (uint64_t)step) * 0x100000001B3ULL + (uint64_t)(site + 1) * 0x9E3779B97F4A7C15ULL;
}
__global__ __launch_bounds__(1024) void decode_replay_init_kernel(int* __restrict__ step, uint64_t* __restrict__ seeds,
                                                                  float* __restrict__ cur_feat, long n_feat,
                                                                  float* __restrict__ pe_cur, const float* __restrict__ pe_alpha,
                                                                  int Cd, uint64_t seed0) {
  const int tid = threadIdx.x;
  for (long i = tid; i < n_feat; i += 1024) cur_feat[i] = 0.f;  // the zero frame (speech_generator_for_s2st.py:76-77)
  for (int c = tid; c < Cd; c += 1024) pe_cur[c] = pe_alpha[2L * Cd + c];
  if (tid < 8) seeds[tid] = replay_site_seed(seed0, 0, tid);
  if (tid == 0) *step = 0;
}
// Commit of a replayed step.  Workgroup 0: the stop rule of decode_stop_update_kernel on the step's probabilities (+ the
// step's row of eos_all), the next step's position row and seeds; the other workgroups: the step's features / alignment into
// row `step` of the run's buffers.  Every workgroup only READS the step counter: decode_replay_advance_kernel, the next node
// of the stream, increments it (one workgroup copying 37 k floats by itself cost 60 us per step).
__global__ __launch_bounds__(256) void decode_replay_commit_kernel(const int* __restrict__ step_p, uint64_t* __restrict__ seeds,
                                                                   const float* __restrict__ cur_feat,
                                                                   const float* __restrict__ cur_eos,
                                                                   const float* __restrict__ cur_attn, float* __restrict__ pe_cur,
                                                                   const float* __restrict__ pe_alpha, int pe_rows, int Cd,
                                                                   uint64_t seed0, float thr, int max_iter, int B, int out_dim, int E,
                                                                   int* __restrict__ finished, int* __restrict__ out_lens,
                                                                   int* __restrict__ klen_next, int* __restrict__ n_done,
                                                                   float* __restrict__ feat_all, float* __restrict__ eos_all,
                                                                   float* __restrict__ attn_all) {
  const int tid = threadIdx.x, step = *step_p;
  if (blockIdx.x == 0) {
    __shared__ int cnt[4];
    int c = 0;
    for (int b = tid; b < B; b += 256) {
      const float pr = cur_eos[b];
      const int cur = pr > thr ? 1 : 0;
      int f = finished[b], ol = out_lens[b];
      if (!f && cur) ol = step + 1;
      f |= cur;
      finished[b] = f;
      out_lens[b] = ol;
      klen_next[b] = ol == max_iter ? step + 2 : ol;
      c += f;
      if (step < max_iter) eos_all[(long)step * B + b] = pr;
    }
    c = (int)wave_sum((float)c);
    if ((tid & 63) == 0) cnt[tid >> 6] = c;
    const int row = min(step + 3, pe_rows - 1);  // next step's position: (step + 1) + 2
    for (int k = tid; k < Cd; k += 256) pe_cur[k] = pe_alpha[(long)row * Cd + k];
    if (tid < 8) seeds[tid] = replay_site_seed(seed0, step + 1, tid);
    __syncthreads();
    if (tid == 0 && step < max_iter) n_done[step] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    return;
  }
  if (step >= max_iter) return;
  const long nf = (long)B * out_dim, na = (attn_all && cur_attn) ? (long)B * E : 0;
  const long i = ((long)blockIdx.x - 1) * 256 + tid;
  if (i < nf) feat_all[(long)step * nf + i] = cur_feat[i];
  else if (i - nf < na) attn_all[(long)step * na + (i - nf)] = cur_attn[i - nf];
}
__global__ void decode_replay_advance_kernel(int* __restrict__ step_p) { *step_p += 1; }
}  // namespace

int s2st_decode_replay_init(int* step, uint64_t* seeds, float* cur_feat, long n_feat, float* pe_cur, const float* pe_alpha, int Cd,
                            uint64_t seed0, hipStream_t st) {
  if (!step || !seeds || !cur_feat || !pe_cur || !pe_alpha || n_feat <= 0 || Cd <= 0) return S2ST_ERR_ARG;
  S2ST_LAUNCH(decode_replay_init_kernel, dim3(1), dim3(1024), 0, st, step, seeds, cur_feat, n_feat, pe_cur, pe_alpha, Cd, seed0);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
int s2st_decode_replay_commit(int* step, uint64_t* seeds, const float* cur_feat, const float* cur_eos, const float* cur_attn,
                              float* pe_cur, const float* pe_alpha, int pe_rows, int Cd, uint64_t seed0, float thr, int max_iter,
                              int B, int out_dim, int E, int* finished, int* out_lens, int* klen_next, int* n_done,
                              float* feat_all, float* eos_all, float* attn_all, hipStream_t st) {
  if (B <= 0) return 0;
  if (!step || !seeds || !cur_feat || !cur_eos || !pe_cur || !pe_alpha || !finished || !out_lens || !klen_next || !n_done ||
      !feat_all || !eos_all)
    return S2ST_ERR_ARG;
  const long n_copy = (long)B * out_dim + ((attn_all && cur_attn) ? (long)B * E : 0);
  S2ST_LAUNCH(decode_replay_commit_kernel, dim3(1 + (unsigned)((n_copy + 255) / 256)), dim3(256), 0, st, (const int*)step, seeds,
              cur_feat, cur_eos, cur_attn, pe_cur, pe_alpha, pe_rows, Cd, seed0, thr, max_iter, B, out_dim, E, finished, out_lens,
              klen_next, n_done, feat_all, eos_all, attn_all);
  S2ST_LAUNCH(decode_replay_advance_kernel, dim3(1), dim3(1), 0, st, step);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_decode_stop_update(const float* eos_prob, float thr, int step, int max_iter, int B, int* finished, int* out_lens,
                            int* klen_next, int* n_done, hipStream_t st) {
  if (B <= 0) return 0;
  if (!eos_prob || !finished || !out_lens || !klen_next || !n_done || step < 0) return S2ST_ERR_ARG;
  S2ST_LAUNCH(decode_stop_update_kernel, dim3(1), dim3(256), 0, st, eos_prob, thr, step, max_iter, B, finished, out_lens, klen_next,
              n_done);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_sigmoid(const float* x, float* y, long n, hipStream_t st) {
  if (n <= 0) return 0;
  S2ST_LAUNCH(sigmoid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, n);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_argmax_dim1(const float* x, long* idx, int B, int E, int D, hipStream_t st) {
  const long n = (long)B * D;
  if (n <= 0 || E <= 0) return 0;
  S2ST_LAUNCH(argmax_dim1_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, idx, B, E, D);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_affine_cols(const float* x, const float* scale, const float* shift, float* y, long rows, int C,
                     hipStream_t st) {
  const long n = rows * C;
  if (n <= 0) return 0;
  S2ST_LAUNCH(affine_cols_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, scale, shift, y, rows,
                     C);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
