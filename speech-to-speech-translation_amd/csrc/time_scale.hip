// Time-scale modification of 16-bit PCM: the tempo of speech changes, its pitch does not.  Waveform-similarity overlap-add on
// integers; the reference has no counterpart, the definition is in include/s2st_hip.h (s2st_time_scale_pcm16) and is restated,
// operation for operation, by time_scale.host_time_scale.  Everything is integer and exact, so the two agree bit for bit.
//
// ts_wsola_kernel: one 256-thread workgroup per recording walks the hops (hop j needs the position hop j - 1 chose).  Per hop:
//   * the samples x[a_j - D .. a_j + D + 2 Hs) lie in LDS as 16-bit values with 32768 added (|a - b| is the same and both
//     operands are unsigned): the candidates' windows, the samples the output is blended from and the next hop's template are
//     all inside that region, so the hop reads nothing from global memory.  The region needs a_j only, not the choice: the
//     next hop's region is fetched into registers before this hop is scored and lands in LDS behind the hop's last barrier.
//     The barriers between wait for LDS only (ts_lds_barrier), so that fetch stays in flight across them;
//   * a work item is four consecutive candidates (the first at a multiple of four) times a slice of the template; it slides
//     a window of four dwords over the region, two new dwords (one ds_read_b64) and one template ds_read_b64 (a broadcast)
//     per step of four samples, and adds eight packed sums of absolute differences (v_sad_u16: two terms and the accumulate
//     in one instruction).  The candidates at odd offsets straddle the packed pairs: their dwords come either from a funnel
//     shift of two neighbouring dwords (two v_perm_b32 per step) or from a second LDS image of the region shifted by one
//     sample (one more ds_read_b64 per step) -- ts_wsola_kernel<false> / <true>.  The funnel shift measured faster
//     (profiles/time_scale_rate.txt) and is what s2st_time_scale_pcm16 launches; S2ST_TS_ODD=funnel|image selects either for
//     that measurement and for the tests of both;
//   * the partial costs of the slices go through LDS; a thread per candidate adds them (and the up to three samples that fill
//     no step), forms one key -- cost, then |c - a_j|, then c -- and the smallest key is found with wave shuffles and one LDS
//     exchange.  No atomics, nothing read back: the result repeats bit for bit and does not depend on the batch.
#include "s2st_ops.h"
#include "s2st_prof.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_MAX_N = 4096, TS_MAX_D = 2048;
constexpr int TS_SLACK = 16;     // samples behind the region that the phantom candidates of the last work item may read
constexpr int TS_PRE = 16;       // dwords of the next region a thread holds in registers: 256 x 16 x 2 = 8192 = 2 D + 2 Hs at most

// |a.lo - b.lo| + |a.hi - b.hi| + acc over the two unsigned 16-bit halves
#if defined(__AMDGCN__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_sad_u16)
#define TS_HAVE_SAD_U16 1
#endif
#endif
__device__ __forceinline__ unsigned ts_sad(unsigned a, unsigned b, unsigned acc) {
#ifdef TS_HAVE_SAD_U16
  return __builtin_amdgcn_sad_u16(a, b, acc);
#else
  const int d0 = (int)(a & 0xffffu) - (int)(b & 0xffffu), d1 = (int)(a >> 16) - (int)(b >> 16);
  return acc + (unsigned)(d0 < 0 ? -d0 : d0) + (unsigned)(d1 < 0 ? -d1 : d1);
#endif
}
// the dword that starts one sample behind `lo`
__device__ __forceinline__ unsigned ts_funnel(unsigned lo, unsigned hi) { return (lo >> 16) | (hi << 16); }

// LDS, in 16-bit samples: the region (and its image), the template, then the partial costs as int32
__host__ __device__ inline int ts_region_len(int Hs, int D) { return (2 * D + 2 * Hs + TS_SLACK + 7) & ~7; }
__host__ __device__ inline int ts_tpl_len(int Hs) { return (Hs + 7) & ~7; }
__host__ __device__ inline int ts_groups(int D) { return (2 * D + 1 + 3) / 4; }
__host__ __device__ inline int ts_slices(int D) { const int s = TS_THREADS / ts_groups(D); return s < 1 ? 1 : s; }
inline unsigned ts_lds_bytes(int Hs, int D, bool image) {
  return (unsigned)(((image ? 2 : 1) * ts_region_len(Hs, D) + ts_tpl_len(Hs)) * 2 + ts_slices(D) * ts_groups(D) * 4 * 4);
}

// lgkmcnt(0) -- my LDS reads and writes are done -- and a raw s_barrier; global traffic stays in flight
__device__ __forceinline__ void ts_lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
}

template <bool IMAGE>
__global__ __launch_bounds__(TS_THREADS) void ts_wsola_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ ioff,
                                                              const int64_t* __restrict__ ooff, const int64_t* __restrict__ poff,
                                                              int N, int D, int16_t* __restrict__ out, int* __restrict__ pos) {
  HIP_DYNAMIC_SHARED(float4, smem4)  // (float4: the base is 16-byte aligned)
  __shared__ unsigned long long red[TS_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Hs = N / 2, C = 2 * D + 1, G = ts_groups(D), S = ts_slices(D);
  const int F = Hs / 4;                   // whole steps of four samples; the samples [4 F, Hs) are added by the reduction
  const int Ld = 2 * D + 2 * Hs, Lr = ts_region_len(Hs, D), Lt = ts_tpl_len(Hs);
  uint16_t* R = reinterpret_cast<uint16_t*>(smem4);  // R[i] = x[a_j - D + i] + 32768
  uint16_t* I = R + Lr;                              // I[i] = R[i + 1]            (IMAGE only)
  uint16_t* T = R + (IMAGE ? 2 : 1) * Lr;            // the template + 32768
  int* part = reinterpret_cast<int*>(T + Lt);        // part[s][k]: slice s of candidate k's cost, k < 4 G
  unsigned* R32 = reinterpret_cast<unsigned*>(R);
  unsigned* I32 = reinterpret_cast<unsigned*>(I);

  const int64_t n = max((int64_t)0, ioff[b + 1] - ioff[b]), m = max((int64_t)0, ooff[b + 1] - ooff[b]);
  const int64_t J = (m + Hs - 1) / Hs, pcap = poff[b + 1] - poff[b];
  const int16_t* x = pcm + ioff[b];
  int16_t* y = out + ooff[b];
  int* ps = pos + poff[b];
  auto at = [&](int64_t t) -> unsigned {  // x[t] + 32768; 0 + 32768 outside the recording
    return (t >= 0 && t < n) ? (unsigned)((uint16_t)x[t] ^ 0x8000u) : 0x8000u;
  };

  // the region of hop j into registers: dword q = the samples 2 q, 2 q + 1 (and, for the image, 2 q + 1, 2 q + 2)
  unsigned pre[TS_PRE], prei[IMAGE ? TS_PRE : 1];
  auto fetch = [&](int64_t a) {  // a = a_j
    const int64_t base = a - D;
#pragma unroll
    for (int u = 0; u < TS_PRE; ++u) {
      const int q = tid + u * TS_THREADS;
      if (2 * q < Ld) {
        const unsigned s0 = at(base + 2 * q), s1 = at(base + 2 * q + 1);
        pre[u] = s0 | (s1 << 16);
        if constexpr (IMAGE) prei[u] = s1 | (at(base + 2 * q + 2) << 16);
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < TS_PRE; ++u) {
      const int q = tid + u * TS_THREADS;
      if (2 * q < Ld) {
        R32[q] = pre[u];
        if constexpr (IMAGE) I32[q] = prei[u];
      }
    }
  };

  // hop 0: the input as it is; the first template is its continuation
  for (int i = tid; i < Hs && i < m; i += TS_THREADS) y[i] = i < n ? x[i] : (int16_t)0;
  if (tid == 0 && J > 0 && pcap > 0) ps[0] = 0;
  if (J <= 1) return;  // (workgroup-uniform)
  for (int i = tid; i < Lt; i += TS_THREADS) T[i] = (uint16_t)(i < Hs ? at((int64_t)Hs + i) : 0x8000u);
  for (int i = Ld + tid; i < Lr; i += TS_THREADS) {
    R[i] = 0x8000u;
    if constexpr (IMAGE) I[i] = 0x8000u;
  }
  // this thread's cross-fade weights: wr of the samples tid, tid + 256, ..  (Hs <= 2048: eight at most)
  int wrv[TS_MAX_N / 2 / TS_THREADS];
#pragma unroll
  for (int u = 0; u < TS_MAX_N / 2 / TS_THREADS; ++u) wrv[u] = ((2 * (tid + u * TS_THREADS) + 1) * 32768) / N;
  int64_t a = ((int64_t)Hs * n) / m, a_next = 0;  // a_1
  fetch(a);
  commit();
  __syncthreads();

  for (int64_t j = 1; j < J; ++j, a = a_next) {
    if (j + 1 < J) {
      a_next = ((j + 1) * Hs * n) / m;
      fetch(a_next);  // in flight until the commit below
    }

    // ---- the costs: part[s][k0 .. k0 + 3] over the steps of slice s
    for (int w = tid; w < G * S; w += TS_THREADS) {
      const int g = w % G, s = w / G;
      const int f0 = (int)((long)s * F / S), f1 = (int)((long)(s + 1) * F / S);
      unsigned c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      if (f0 < f1) {
        const uint2* Rp = reinterpret_cast<const uint2*>(R32 + 2 * g);  // the dwords from candidate k0 = 4 g on
        const uint2* Ip = reinterpret_cast<const uint2*>(I32 + 2 * g);
        const uint2* Tp = reinterpret_cast<const uint2*>(T);
        uint2 r = Rp[f0];  // r.x, r.y: the window's first two dwords
        unsigned q0, q1 = 0;
        if constexpr (IMAGE) {
          const uint2 q = Ip[f0];
          q0 = q.x;
          q1 = q.y;
        } else {
          q0 = ts_funnel(r.x, r.y);
        }
#pragma unroll 4
        for (int f = f0; f < f1; ++f) {
          const uint2 t = Tp[f], rn = Rp[f + 1];
          unsigned q2;
          if constexpr (IMAGE) {
            const uint2 qn = Ip[f + 1];
            c1 = ts_sad(q0, t.x, c1);
            c1 = ts_sad(q1, t.y, c1);
            c3 = ts_sad(q1, t.x, c3);
            c3 = ts_sad(qn.x, t.y, c3);
            q0 = qn.x;
            q1 = qn.y;
          } else {
            q1 = ts_funnel(r.y, rn.x);
            q2 = ts_funnel(rn.x, rn.y);
            c1 = ts_sad(q0, t.x, c1);
            c1 = ts_sad(q1, t.y, c1);
            c3 = ts_sad(q1, t.x, c3);
            c3 = ts_sad(q2, t.y, c3);
            q0 = q2;
          }
          c0 = ts_sad(r.x, t.x, c0);
          c0 = ts_sad(r.y, t.y, c0);
          c2 = ts_sad(r.y, t.x, c2);
          c2 = ts_sad(rn.x, t.y, c2);
          r = rn;
        }
      }
      int4 c;
      c.x = (int)c0, c.y = (int)c1, c.z = (int)c2, c.w = (int)c3;
      *reinterpret_cast<int4*>(part + (s * G + g) * 4) = c;
    }
    ts_lds_barrier();

    // ---- the choice: the smallest (cost, |c - a_j|, c) -- cost < 2^27, the other two < 2^13
    unsigned long long best = ~0ull;
    for (int k = tid; k < C; k += TS_THREADS) {
      unsigned cost = 0;
      for (int s = 0; s < S; ++s) cost += (unsigned)part[s * G * 4 + k];
      for (int i = 4 * F; i < Hs; ++i) {
        const int d = (int)R[k + i] - (int)T[i];
        cost += (unsigned)(d < 0 ? -d : d);
      }
      const unsigned long long key = ((unsigned long long)cost << 26) | ((unsigned long long)(k < D ? D - k : k - D) << 13) |
                                     (unsigned long long)k;
      best = key < best ? key : best;
    }
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long other = __shfl_down(best, o);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    ts_lds_barrier();
    best = red[0];
    for (int v = 1; v < TS_THREADS / 64; ++v) best = red[v] < best ? red[v] : best;
    const int kb = (int)(best & 0x1fffu);
    if (tid == 0 && j < pcap) ps[j] = (int)(a - D + kb);

    // ---- the output of this hop and the template of the next (thread i reads T[i] before it replaces it)
#pragma unroll
    for (int u = 0; u < TS_MAX_N / 2 / TS_THREADS; ++u) {
      const int i = tid + u * TS_THREADS;
      if (i < Hs) {
        const int xr = (int)R[kb + i] - 32768, xt = (int)T[i] - 32768;
        const int64_t idx = j * Hs + i;
        if (idx < m) y[idx] = (int16_t)((xr * wrv[u] + xt * (32768 - wrv[u]) + 16384) >> 15);
        T[i] = R[kb + Hs + i];
      }
    }
    ts_lds_barrier();  // (every read of the region is done)
    if (j + 1 < J) commit();
    ts_lds_barrier();
  }
}

}  // namespace

int s2st_time_scale_wsola(const int16_t* pcm, const int64_t* in_off, const int64_t* out_off, int B, int N, int D, int16_t* out,
                          int* pos, const int64_t* pos_off, hipStream_t st) {
  if (N < 2 || N > TS_MAX_N || (N & 1) || D < 0 || D > TS_MAX_D || B < 0) return S2ST_ERR_ARG;
  if (B == 0) return 0;
  if (!pcm || !in_off || !out_off || !out || !pos || !pos_off) return S2ST_ERR_ARG;
  // the odd offsets: the funnel shift, unless the measurement asks for the second image
  const char* e = getenv("S2ST_TS_ODD");
  const bool image = e && !strcmp(e, "image");
  const unsigned lds = ts_lds_bytes(N / 2, D, image);
  if (image)
    S2ST_LAUNCH(ts_wsola_kernel<true>, dim3((unsigned)B), dim3(TS_THREADS), lds, st, pcm, in_off, out_off, pos_off, N, D, out, pos);
  else
    S2ST_LAUNCH(ts_wsola_kernel<false>, dim3((unsigned)B), dim3(TS_THREADS), lds, st, pcm, in_off, out_off, pos_off, N, D, out, pos);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
