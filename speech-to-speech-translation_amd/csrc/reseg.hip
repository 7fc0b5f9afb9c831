// Minimum-error re-segmentation: cut a recording's hypothesis words where their least-edit-distance alignment to the
// concatenated reference sentences crosses each sentence boundary.  The reference has no counterpart; the definition is in
// include/s2st_hip.h (s2st_reseg_i32) and is restated by resegment.host_resegment in the OTHER formulation (back-pointers and
// a walk back); everything is integer and exact, so the two agree bit for bit.
//
// rs_kernel: one workgroup per document.
//   * prologue: the clamped segment ends (a running maximum over `ends`, cut at m, the last one m) and, per reference column,
//     the first k that ends there (-1: no boundary) go to the workspace;
//   * the table is walked as a skewed wavefront.  A thread owns a strip of RS_C reference columns and keeps D[i-1][.] and
//     carry(i-1, .) of the strip, the reference ids and the boundary marks in registers; at step s thread t does hypothesis row
//     s - t + 1.  The strip's left edge -- D and carry of the neighbouring column, packed into one dword (both < 2^15) --
//     comes from the lane below by one wave shuffle, for the first lane of a wave through LDS (two slots per wave, taken in
//     turn, so one barrier per step is enough; the barrier waits for LDS only).  The hypothesis ids (and, for the first
//     thread, the left edge of the column block) lie in an LDS ring of two chunks of THREADS rows; the next chunk is fetched
//     into a register THREADS steps ahead and lands in the ring behind the last step that reads the chunk it replaces.  A
//     reference longer than THREADS x RS_C columns is done in column blocks: the last thread leaves its edge per row in the
//     workspace and the first thread of the next block takes it from there;
//   * carry(i, j) is the row at which the walk back from (i, j) first reaches the nearest boundary column < j (column 0 counts
//     as one), so no per-cell back-pointers are kept: at a boundary column e the dword D[i][e] << 16 | carry(i, e) is stored
//     for every row i (the crossing table);
//   * epilogue: one lane follows the K boundaries down from (n, m): one dependent load each gives the distance there and the
//     cut at the boundary before.  No atomics, nothing read back: the result repeats bit for bit and does not depend on the
//     batch.
#include "s2st_ops.h"
#include "s2st_prof.h"

#include <cstdlib>
#include <cstring>

namespace {

constexpr int RS_C = 8;            // reference columns per thread
constexpr int RS_MAX = 32767;      // tokens per side at most: D and carry share a dword

struct RsWorkspace {
  long edge, ce, colk, cross, bytes;  // (offsets in int32 elements; bytes in all)
};
inline RsWorkspace rs_workspace(long B, long Nmax, long Mmax, long Kmax) {
  RsWorkspace l;
  l.edge = 0;
  l.ce = l.edge + B * (Nmax + 1);
  l.colk = l.ce + B * Kmax;
  l.cross = l.colk + B * (Mmax + 1);
  l.bytes = (l.cross + B * Kmax * (Nmax + 1)) * 4;
  return l;
}

// lgkmcnt(0) -- my LDS reads and writes are done -- and a raw s_barrier; global traffic stays in flight
__device__ __forceinline__ void rs_lds_barrier() {
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();
}
__device__ __forceinline__ int rs_pack(int d, int c) { return (int)(((unsigned)d << 16) | (unsigned)c); }

template <int THREADS>
__global__ __launch_bounds__(THREADS) void rs_kernel(const int* __restrict__ hyp, const int64_t* __restrict__ hoff,
                                                     const int* __restrict__ ref, const int64_t* __restrict__ roff,
                                                     const int* __restrict__ ends, const int64_t* __restrict__ eoff, int Nmax,
                                                     int Mmax, int Kmax, int* __restrict__ cuts, int* __restrict__ seg_dist,
                                                     int* __restrict__ dist, int* ws, RsWorkspace L) {
  constexpr int WAVES = THREADS / 64, RING = 2 * THREADS, W = THREADS * RS_C;
  __shared__ int hring[RING];         // hypothesis ids of two chunks of THREADS rows
  __shared__ int ering[RING];         // the column block's left edge of the same rows (row index + 1)
  __shared__ int slot[2][WAVES];      // the last lane's edge of every wave, two steps deep
  __shared__ int pmax[THREADS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = (int)min((int64_t)Nmax, max((int64_t)0, hoff[b + 1] - hoff[b]));
  const int m = (int)min((int64_t)Mmax, max((int64_t)0, roff[b + 1] - roff[b]));
  const int K = (int)min((int64_t)Kmax, max((int64_t)0, eoff[b + 1] - eoff[b]));
  const int* h = hyp + hoff[b];
  const int* r = ref + roff[b];
  const int* en = ends + eoff[b];
  const long N1 = (long)Nmax + 1;
  int* edge = ws + L.edge + (long)b * N1;
  int* ce = ws + L.ce + (long)b * Kmax;
  int* colk = ws + L.colk + (long)b * ((long)Mmax + 1);
  int* cross = ws + L.cross + (long)b * Kmax * N1;

  // ---- the clamped ends: e_k = min(max(0, ends[0..k]), m), the last one m; colk[j] = the first k with e_k = j
  {
    const int per = (K + THREADS - 1) / THREADS, k0 = min(K, tid * per), k1 = min(K, k0 + per);
    int run = 0;
    for (int k = k0; k < k1; ++k) run = max(run, en[k]);
    pmax[tid] = run;
    for (int j = tid; j <= m; j += THREADS) colk[j] = -1;
    __syncthreads();
    run = 0;
    for (int t = 0; t < tid; ++t) run = max(run, pmax[t]);
    for (int k = k0; k < k1; ++k) {
      run = max(run, en[k]);
      ce[k] = k == K - 1 ? m : min(run, m);
    }
    __syncthreads();
    for (int k = tid; k < K; k += THREADS) {
      const int e = ce[k];
      if (k == 0 || ce[k - 1] != e) colk[e] = k;
    }
    __syncthreads();
  }
  if (m == 0 && tid == 0) dist[b] = n;

  // ---- the table, a block of W columns at a time
  for (int base = 0; base < m; base += W) {
    const int strips = (min(W, m - base) + RS_C - 1) / RS_C;
    const bool more = base + W < m;          // another block follows: the last thread leaves its edge
    const int j0 = base + tid * RS_C;        // the column left of the strip; the strip is j0 + 1 .. j0 + RS_C
    const bool mine = tid < strips;
    int rid[RS_C], kk[RS_C], Dp[RS_C], Cp[RS_C];
    unsigned lb = 0;                         // bit c: column j0 + c is a boundary (or column 0): a step from j0 + c + 1 into it
#pragma unroll
    for (int c = 0; c < RS_C; ++c) {
      const int j = j0 + c + 1;
      const bool ok = mine && j <= m;
      rid[c] = ok ? r[j - 1] : 0;
      kk[c] = ok ? colk[j] : -1;
      const bool left = mine && j - 1 <= m && (j - 1 == 0 || colk[j - 1] >= 0);
      lb |= (left ? 1u : 0u) << c;
      Dp[c] = j;  // row 0
      Cp[c] = 0;
      if (kk[c] >= 0) cross[(long)kk[c] * N1] = rs_pack(j, 0);
    }
    int diag = rs_pack(j0, 0);               // D[i-1][j0], carry(i-1, j0): the left edge of the row before
    int out = rs_pack(Dp[RS_C - 1], 0);      // what the neighbour gets: my right edge of the row just done
    // chunk 0 of the ring, chunk 1 into registers
    auto fetch_h = [&](int q) { const int idx = q * THREADS + tid; return idx < n ? h[idx] : 0; };
    auto fetch_e = [&](int q) { const int idx = q * THREADS + tid; return (base > 0 && idx < n) ? edge[idx + 1] : 0; };
    hring[tid] = fetch_h(0);
    ering[tid] = fetch_e(0);
    int nh = fetch_h(1), ne = fetch_e(1);
    __syncthreads();

    const int steps = n > 0 ? n + strips - 1 : 0;
    for (int s = 0; s < steps; ++s) {
      const int idx = s - tid;               // this thread's hypothesis word; its row is idx + 1
      const bool act = mine && idx >= 0 && idx < n;
      int left = __shfl(out, lane - 1);
      if (lane == 0 && wave > 0) left = slot[(s + 1) & 1][wave - 1];
      if (act) {
        const int i = idx + 1;
        const int hv = hring[idx & (RING - 1)];
        if (tid == 0) left = base > 0 ? ering[idx & (RING - 1)] : rs_pack(i, 0);
        int dl = left >> 16, cl = left & 0xffff, dd = diag >> 16, cd = diag & 0xffff;
#pragma unroll
        for (int c = 0; c < RS_C; ++c) {
          const bool bnd = (lb >> c) & 1u;
          const int ud = Dp[c], uc = Cp[c];
          int best = dd + (hv != rid[c] ? 1 : 0), bc = bnd ? i - 1 : cd;  // the diagonal first,
          if (ud + 1 < best) best = ud + 1, bc = uc;                        // then up,
          if (dl + 1 < best) best = dl + 1, bc = bnd ? i : cl;              // then left
          dd = ud, cd = uc;
          Dp[c] = dl = best;
          Cp[c] = cl = bc;
          if (kk[c] >= 0) cross[(long)kk[c] * N1 + i] = rs_pack(best, bc);
        }
        diag = left;
        out = rs_pack(dl, cl);
        if (more && tid == THREADS - 1) edge[i] = out;
      }
      if (lane == 63) slot[s & 1][wave] = out;
      if ((s & (THREADS - 1)) == THREADS - 1) {  // the chunk this one replaces was last read a step ago
        const int q = s / THREADS + 1;
        hring[(q & 1) * THREADS + tid] = nh;
        ering[(q & 1) * THREADS + tid] = ne;
        nh = fetch_h(q + 1);
        ne = fetch_e(q + 1);
      }
      rs_lds_barrier();
    }
    if (!more) {  // D[n][m]
      const int jm = m - base - 1;
      if (tid == jm / RS_C) {
        int d = 0;
#pragma unroll
        for (int c = 0; c < RS_C; ++c) d = (jm % RS_C == c) ? Dp[c] : d;
        dist[b] = d;
      }
    }
    __syncthreads();  // the edges and the crossing table are written; the ring is free
  }

  // ---- the cuts: from (n, m) down the boundaries
  if (tid == 0) {
    int c = n, y_next = 0, below = 0, e_next = -1;
    for (int k = K - 1; k >= 0; --k) {
      const int e = ce[k];
      int y = y_next;
      if (e != e_next) {  // a new column: the cut there, the distance there and the cut at the boundary before
        if (k < K - 1) c = below;
        if (e == 0) {
          y = c;
        } else {
          const int v = cross[(long)colk[e] * N1 + c];
          y = v >> 16;
          below = v & 0xffff;
        }
      }
      cuts[eoff[b] + k] = c;
      if (k < K - 1) seg_dist[eoff[b] + k + 1] = y_next - y;
      y_next = y;
      e_next = e;
    }
    if (K > 0) seg_dist[eoff[b]] = y_next;
  }
}

}  // namespace

int64_t s2st_reseg_ws_bytes(int B, int Nmax, int Mmax, int Kmax) {
  if (B < 0 || Nmax < 0 || Mmax < 0 || Kmax < 0) return S2ST_ERR_ARG;
  return rs_workspace(B, Nmax, Mmax, Kmax).bytes;
}

int s2st_reseg_align(const int* hyp, const int64_t* hoff, const int* ref, const int64_t* roff, const int* ends,
                     const int64_t* eoff, int B, int Nmax, int Mmax, int Kmax, int* cuts, int* seg_dist, int* dist,
                     void* workspace, int64_t workspace_bytes, hipStream_t st) {
  if (B < 0 || Nmax < 0 || Mmax < 0 || Kmax < 0) return S2ST_ERR_ARG;
  if (B == 0) return 0;
  if (!hyp || !hoff || !ref || !roff || !ends || !eoff || !cuts || !seg_dist || !dist) return S2ST_ERR_ARG;
  if (Nmax > RS_MAX || Mmax > RS_MAX) return S2ST_ERR_SHAPE;
  const RsWorkspace L = rs_workspace(B, Nmax, Mmax, Kmax);
  if (!workspace || workspace_bytes < L.bytes) return S2ST_ERR_ARG;
  // the width of the wavefront: 1024 threads (8192 columns a block) measured faster than 256 on documents of 2000 to 6000
  // tokens (profiles/resegment_rate.txt); S2ST_RESEG_THREADS=256|1024 selects either for that measurement and the tests of both
  const char* e = getenv("S2ST_RESEG_THREADS");
  if (e && !strcmp(e, "256"))
    S2ST_LAUNCH(rs_kernel<256>, dim3((unsigned)B), dim3(256), 0, st, hyp, hoff, ref, roff, ends, eoff, Nmax, Mmax, Kmax, cuts,
                seg_dist, dist, (int*)workspace, L);
  else
    S2ST_LAUNCH(rs_kernel<1024>, dim3((unsigned)B), dim3(1024), 0, st, hyp, hoff, ref, roff, ends, eoff, Nmax, Mmax, Kmax, cuts,
                seg_dist, dist, (int*)workspace, L);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
