// Pause-seeking segmentation of long recordings: where to cut a recording that is longer than the model takes.  The
// reference has no counterpart (it only ever sees utterances); the definition is in include/s2st_hip.h (s2st_segment_pcm16)
// and is restated, operation for operation, by segmentation.host_segment.  Everything is int64 and exact, so the two agree
// bit for bit.
//
// seg_energy_kernel: a 256-thread workgroup owns 256 - 2 w frames of one recording and computes the energies of those and of
//   w frames on either side into LDS (a thread per frame), then the smoothed energies from LDS; it leaves E, S and the
//   maxima of its frames in the workspace.  The maxima of a recording are the maxima of its tiles: integer, order-free, no
//   atomics.
// seg_search_kernel: one workgroup per recording.  D[t] needs D[s] for s <= t - min_len only, so the frames t0 .. t0 + min_len
//   - 1 depend on nothing younger than t0 - 1: a step advances min_len frames, a frame per thread, between two barriers (a
//   frame-by-frame loop would pay a barrier per frame).  D lives in an LDS ring of max_len + min_len entries (rounded up to
//   whole chunks); over it lies a second level, the minimum and arg-min of every complete chunk of SG_C entries, so that a
//   thread's scan of its window [t - max_len, t - min_len] reads the head and tail of the window entry by entry and the
//   chunks between them as one value each: O(SG_C + max_len / SG_C) reads.  Scans run upwards and replace on strictly
//   smaller only: ties go to the smallest s.  Back-pointers are int32 in the workspace; the back-trace (one lane), the
//   trimming (a wave per segment: ballots over 64 frames from either end) and the outputs follow in the same launch.
#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

constexpr int SG_C = 32;                  // entries per chunk of the second level
constexpr int SG_BATCH = 8;               // LDS reads in flight per thread in a scan
constexpr int SG_MAX_RING = 7168;        // max_len + min_len at most: ring + chunk level + statics stay under 64 KiB
constexpr int SG_MAX_W = 64;              // smoothing half-width at most: a tile keeps 256 - 2 w >= 128 frames
constexpr int64_t SG_INF = INT64_MAX;     // an unreachable frame; never enters an add

inline long sg_align8(long n) { return (n + 7) & ~7L; }
inline int sg_tiles_cap(int Tmax) { return (Tmax + (256 - 2 * SG_MAX_W) - 1) / (256 - 2 * SG_MAX_W); }
inline int sg_rev_cap(int Tmax, int min_len) { return max(1, Tmax / max(min_len, 1)) + 1; }

struct SgWorkspace {
  long e, s, part, bp, rev, bytes;
};
inline SgWorkspace sg_workspace(int B, int Tmax, int min_len) {
  SgWorkspace l;
  l.e = 0;
  l.s = l.e + (long)B * Tmax * 8;
  l.part = l.s + (long)B * Tmax * 8;
  l.bp = l.part + (long)B * sg_tiles_cap(Tmax) * 2 * 8;
  l.rev = l.bp + sg_align8((long)B * (Tmax + 1) * 4);
  l.bytes = l.rev + sg_align8((long)B * sg_rev_cap(Tmax, min_len) * 4);
  return l;
}

__device__ __forceinline__ int sg_frames(const int64_t* __restrict__ soff, int b, int win, int hop, int Tmax) {
  const int64_t n = soff[b + 1] - soff[b];
  if (n < win) return 0;
  return (int)min((int64_t)Tmax, 1 + (n - win) / hop);
}

// the barrier inside the search: lgkmcnt(0) -- my LDS reads and writes are done -- and a raw s_barrier; global traffic
// stays in flight
__device__ __forceinline__ void sg_lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
}

// floor((double)m * f): one IEEE double multiply and a floor (m < 2^53: the conversion is exact)
__device__ __forceinline__ int64_t sg_scale(int64_t m, double f) {
  const double p = (double)m * f;
  return p >= 4611686018427387904.0 ? (int64_t)1 << 62 : (int64_t)floor(p);
}

__global__ __launch_bounds__(256) void seg_energy_kernel(const int16_t* __restrict__ pcm, const int64_t* __restrict__ soff,
                                                         int Tmax, int win, int hop, int w, int64_t* __restrict__ E,
                                                         int64_t* __restrict__ S, int64_t* __restrict__ part, int tiles_cap) {
  __shared__ int64_t e[256];
  __shared__ int64_t red[2][256];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int F = 256 - 2 * w, tile0 = blockIdx.x * F;
  const int T = sg_frames(soff, b, win, hop, Tmax);
  if (tile0 >= T) return;  // (workgroup-uniform)
  const int f = tile0 - w + tid;
  int64_t en = 0;
  if (f >= 0 && f < T) {
    const int16_t* x = pcm + soff[b] + (int64_t)f * hop;  // the last read is sample f hop + win - 1 <= n - 1
    for (int i = 0; i < win; ++i) {
      const int v = x[i];
      en += (int64_t)(v * v);  // <= 2^30
    }
  }
  e[tid] = en;
  __syncthreads();
  int64_t mE = 0, mS = 0;
  if (tid >= w && tid < 256 - w && f < T) {
    const int lo = max(0, f - w), hi = min(T - 1, f + w);
    int64_t s = 0;
    for (int u = lo; u <= hi; ++u) s += e[u - (tile0 - w)];
    E[(long)b * Tmax + f] = en;
    S[(long)b * Tmax + f] = s;
    mE = en;
    mS = s;
  }
  red[0][tid] = mE;
  red[1][tid] = mS;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (tid < h) {
      red[0][tid] = max(red[0][tid], red[0][tid + h]);
      red[1][tid] = max(red[1][tid], red[1][tid + h]);
    }
    __syncthreads();
  }
  if (tid < 2) part[((long)b * tiles_cap + blockIdx.x) * 2 + tid] = red[tid][0];
}

__global__ __launch_bounds__(256) void seg_search_kernel(const int64_t* __restrict__ soff, int Tmax, int win, int hop, int w,
                                                         int min_len, int max_len, int pad, double penalty_factor,
                                                         double silence_factor, int Kcap, const int64_t* __restrict__ E,
                                                         const int64_t* __restrict__ S, const int64_t* __restrict__ part,
                                                         int tiles_cap, int* bp_all, int* rev_all, int rev_cap,
                                                         int* __restrict__ nseg, int* __restrict__ seg_start,
                                                         int* __restrict__ seg_end, int* __restrict__ trim_start,
                                                         int* __restrict__ trim_end, int* __restrict__ dropped,
                                                         int64_t* __restrict__ cost) {
  HIP_DYNAMIC_SHARED(float4, smem4)  // (float4: the base is 16-byte aligned)
  __shared__ int64_t red[2][256];
  __shared__ int n_seg;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int R = (max_len + min_len + SG_C - 1) / SG_C * SG_C, NC = R / SG_C;
  int64_t* D = reinterpret_cast<int64_t*>(smem4);  // ring: D[s] at s % R
  int64_t* M = D + R;                              // chunk c's minimum at c % NC ..
  int* A = reinterpret_cast<int*>(M + NC);         // .. and its smallest arg-min (-1: no reachable entry)
  const int T = sg_frames(soff, b, win, hop, Tmax);
  E += (long)b * Tmax;
  S += (long)b * Tmax;
  int* bp = bp_all + (long)b * (Tmax + 1);
  int* rev = rev_all + (long)b * rev_cap;

  // the recording's maxima from its tiles' maxima
  {
    const int F = 256 - 2 * w, tiles = (T + F - 1) / F;
    int64_t mE = 0, mS = 0;
    for (int i = tid; i < tiles; i += 256) {
      mE = max(mE, part[((long)b * tiles_cap + i) * 2]);
      mS = max(mS, part[((long)b * tiles_cap + i) * 2 + 1]);
    }
    red[0][tid] = mE;
    red[1][tid] = mS;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
      if (tid < h) {
        red[0][tid] = max(red[0][tid], red[0][tid + h]);
        red[1][tid] = max(red[1][tid], red[1][tid + h]);
      }
      __syncthreads();
    }
  }
  const int64_t thr = sg_scale(red[0][0], silence_factor), lambda = sg_scale(red[1][0], penalty_factor);

  int64_t total = 0;
  if (T >= min_len) {
    int c_done = 0;  // chunks [0, c_done) have their minima
    // One step: frames t0 .. t0 + min_len - 1.  `cur` holds S of this thread's first frame of the step, fetched a step ago;
    // `nxt` receives that of the next step now, so that no step waits for global memory.  The two barriers of a step wait
    // for LDS only (sg_lds_barrier): the back-pointer stores and that fetch stay in flight across them.
    auto step = [&](int t0, const int64_t& cur, int64_t& nxt) {
      const int t_end = min(t0 + min_len, T + 1);
      {
        const int tn = t0 + min_len + tid;
        nxt = (tid < min_len && tn < T) ? S[tn] : 0;
      }
      for (int t = t0 + tid; t < t_end; t += 256) {
        const int64_t sv = t == t0 + tid ? cur : (t < T ? S[t] : 0);  // (min_len > 256: the later frames fetch their own)
        const int64_t add = (t > 0 && t < T) ? sv + lambda : 0;       // (the step to T adds no cut cost)
        int64_t best = SG_INF;
        int arg = -1;
        const int hi = t - min_len, lo = max(0, t - max_len);
        // A scan reads SG_BATCH entries at once (independent ds_reads, one wait) and then compares them in order; an index
        // past the run's end is clamped to its last entry, whose second reading never replaces the first (strict <).
        auto run = [&](const int64_t* __restrict__ v, const int* __restrict__ a, int s0, int n) {  // n entries, upwards
          for (int j = 0; j < n; j += SG_BATCH) {
            int64_t d[SG_BATCH];
            int at[SG_BATCH];
#pragma unroll
            for (int u = 0; u < SG_BATCH; ++u) {
              const int k = min(j + u, n - 1);
              d[u] = v[k];
              at[u] = a ? a[k] : s0 + k;
            }
#pragma unroll
            for (int u = 0; u < SG_BATCH; ++u)
              if (d[u] < best) { best = d[u]; arg = at[u]; }
          }
        };
        auto raw = [&](int from, int to) {  // entries [from, to) of D: at most two runs, the ring wraps once
          if (from >= to) return;
          const int i = from % R, n = to - from, first = min(n, R - i);
          run(D + i, nullptr, from, first);
          if (n > first) run(D, nullptr, from + first, n - first);
        };
        if (hi >= 0) {
          const int cf = (lo + SG_C - 1) / SG_C, cl = (hi + 1) / SG_C;  // whole chunks [cf, cl) lie inside the window
          if (cf >= cl) {
            raw(lo, hi + 1);
          } else {
            raw(lo, cf * SG_C);
            const int i = cf % NC, n = cl - cf, first = min(n, NC - i);
            run(M + i, A + i, 0, first);
            if (n > first) run(M, A, 0, n - first);
            raw(cl * SG_C, hi + 1);
          }
        }
        D[t % R] = t == 0 ? 0 : (best == SG_INF ? SG_INF : best + add);
        bp[t] = arg;
      }
      sg_lds_barrier();
      const int c_new = t_end / SG_C;
      for (int c = c_done + tid; c < c_new; c += 256) {
        int64_t best = SG_INF;
        int arg = -1;
        const int i0 = (c % NC) * SG_C;  // (R is a whole number of chunks: a chunk does not wrap)
        for (int j = 0; j < SG_C; ++j) {
          const int64_t d = D[i0 + j];
          if (d < best) { best = d; arg = c * SG_C + j; }
        }
        M[c % NC] = best;
        A[c % NC] = arg;
      }
      c_done = max(c_done, c_new);
      sg_lds_barrier();
    };
    // (two steps per trip, the registers changing roles: no copy at the loop's back edge, which would wait for the fetch)
    int64_t sa = (tid > 0 && tid < T && tid < min_len) ? S[tid] : 0, sb = 0;
    for (int t0 = 0; t0 <= T; t0 += min_len) {
      step(t0, sa, sb);
      t0 += min_len;
      if (t0 > T) break;  // (workgroup-uniform)
      step(t0, sb, sa);
    }
    total = D[T % R];
    __syncthreads();  // (the back-pointers other threads stored are visible to the back-trace)
  }
  // the back-trace: one lane, a dependent load per cut; rev = b_K, b_{K-1}, .., b_1
  if (tid == 0) {
    int k = 0, t = T;
    if (T >= min_len && total != SG_INF) {
      while (t > 0 && k < rev_cap) {
        rev[k++] = t;
        t = bp[t];
      }
    } else {
      rev[k++] = T;
    }
    n_seg = min(k, Kcap);
    nseg[b] = n_seg;
    cost[b] = total == SG_INF ? 0 : total;
  }
  __syncthreads();
  const int K = n_seg;
  // trimming: a wave per segment; the first / last speech frame from ballots over 64 frames from either end
  const int wave = tid >> 6, lane = tid & 63;
  for (int j = wave; j < K; j += 4) {
    const int start = j == 0 ? 0 : rev[K - j], end = rev[K - 1 - j];
    int first = -1, last = -1;
    for (int base = start; base < end; base += 64) {
      const int f = base + lane;
      const unsigned long long m = __ballot(f < end && E[f] > thr);
      if (m) { first = base + __builtin_ctzll(m); break; }
    }
    if (first >= 0) {
      for (int top = end; top > start; top -= 64) {
        const int f = top - 1 - lane;
        const unsigned long long m = __ballot(f >= start && E[f] > thr);
        if (m) { last = top - 1 - __builtin_ctzll(m); break; }
      }
    }
    if (lane == 0) {
      const long o = (long)b * Kcap + j;
      seg_start[o] = start;
      seg_end[o] = end;
      trim_start[o] = first >= 0 ? max(start, first - pad) : start;
      trim_end[o] = first >= 0 ? min(end, last + 1 + pad) : start;
      dropped[o] = first >= 0 ? 0 : 1;
    }
  }
  for (int j = K + tid; j < Kcap; j += 256) {
    const long o = (long)b * Kcap + j;
    seg_start[o] = seg_end[o] = trim_start[o] = trim_end[o] = -1;
    dropped[o] = 0;
  }
}

}  // namespace

int64_t s2st_segment_ws_bytes(int B, int Tmax, int min_len) {
  if (B <= 0 || Tmax < 0 || min_len < 1) return 0;
  return sg_workspace(B, Tmax, min_len).bytes;
}

int s2st_segment_speech(const int16_t* pcm, const int64_t* soff, int B, int Tmax, int win, int hop, int w, int min_len,
                        int max_len, int pad, double penalty_factor, double silence_factor, int Kcap, int* nseg, int* seg_start,
                        int* seg_end, int* trim_start, int* trim_end, int* dropped, int64_t* cost, void* workspace,
                        int64_t workspace_bytes, hipStream_t st) {
  if (B < 0 || B > 65535 || Tmax < 0 || win < 1 || hop < 1 || w < 0 || w > SG_MAX_W || pad < 0) return S2ST_ERR_ARG;
  if (min_len < 1 || max_len < 2L * min_len) return S2ST_ERR_ARG;
  if (!(penalty_factor >= 0.0) || !(silence_factor >= 0.0) || penalty_factor > 1.7e308 || silence_factor > 1.7e308)
    return S2ST_ERR_ARG;  // (negative, NaN, infinite)
  if (Kcap < max(1, Tmax / min_len)) return S2ST_ERR_ARG;
  if ((long)max_len + min_len > SG_MAX_RING) return S2ST_ERR_SHAPE;
  if (B == 0) return 0;
  if (!soff || !nseg || !seg_start || !seg_end || !trim_start || !trim_end || !dropped || !cost) return S2ST_ERR_ARG;
  if (Tmax > 0 && !pcm) return S2ST_ERR_ARG;
  const SgWorkspace l = sg_workspace(B, Tmax, min_len);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < l.bytes) return S2ST_ERR_ARG;
  unsigned char* ws = (unsigned char*)workspace;
  int64_t* E = (int64_t*)(ws + l.e);
  int64_t* S = (int64_t*)(ws + l.s);
  int64_t* part = (int64_t*)(ws + l.part);
  const int tiles_cap = sg_tiles_cap(Tmax);
  if (Tmax > 0) {
    const int F = 256 - 2 * w;
    S2ST_LAUNCH(seg_energy_kernel, dim3((unsigned)((Tmax + F - 1) / F), (unsigned)B), dim3(256), 0, st, pcm, soff, Tmax, win, hop,
                w, E, S, part, tiles_cap);
  }
  const int R = (max_len + min_len + SG_C - 1) / SG_C * SG_C;
  const unsigned lds = (unsigned)((R * 8 + (R / SG_C) * 12 + 15) & ~15);
  S2ST_LAUNCH(seg_search_kernel, dim3((unsigned)B), dim3(256), lds, st, soff, Tmax, win, hop, w, min_len, max_len, pad,
              penalty_factor, silence_factor, Kcap, (const int64_t*)E, (const int64_t*)S, (const int64_t*)part, tiles_cap,
              (int*)(ws + l.bp), (int*)(ws + l.rev), sg_rev_cap(Tmax, min_len), nseg, seg_start, seg_end, trim_start, trim_end,
              dropped, cost);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
