// CTC forced alignment: the Viterbi path of a GIVEN transcript through a head's log-probabilities (frame -> token, token
// spans, per-token and per-utterance scores).  The reference has no counterpart: it never materialises an alignment, and
// SURVEY.md section 0 item 2 leaves the definition to the build ("greedy arg-max path of lprobs and the Viterbi forced
// alignment; both integer").  The greedy half is ctc_greedy_kernel (w2v_ctc.hip); the sum over all paths is ctc_ab_kernel
// (losses.hip).  This file is the best single path.  The definition (include/s2st_hip.h, s2st_ctc_align_f32) is restated
// operation for operation by ctc_align.host_forced_align, and the two agree bit for bit.
//
// One 256-thread workgroup per utterance; a thread owns the same PER states (tid, tid + 256, ..) at every frame, so their
// emission columns and "may skip" flags sit in registers.  The chain of E frames is serial, so a frame's cost is latency:
//   * d lives double-buffered in LDS behind two -inf guard slots (states 0 and 1 read them as their missing neighbours);
//     a frame is three ds_reads per state, two compares, one add, one ds_write, s_waitcnt lgkmcnt(0) and a raw s_barrier;
//   * the gather of a frame's emissions lp[t][ext s] is issued CA_DEPTH frames ahead into a register ring, so that no frame
//     waits for global memory;
//   * back-pointers are 2 bits; a thread collects 16 frames of a state in one register word and stores it once per 16
//     frames at word[(t >> 4)][s] -- no lane shares a word, no atomics.  The words live in LDS where E * S allows it
//     (route 1: the back-trace, one lane walking E dependent steps, then pays an LDS latency per step) or in the caller's
//     workspace (route 2: a global-load latency per step whenever the state or the 16-frame chunk changes).
// After the back-trace the token scores are summed in frame order, one token per thread.  Results repeat bit for bit.
#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

constexpr int CA_MAXS = 2049;             // 2 * Lmax + 1 <= CA_MAXS
constexpr int CA_DEPTH = 4;               // frames of emissions in flight
constexpr int CA_LDS_MAX = 160 * 1024;    // gfx950: 160 KiB of LDS per workgroup
constexpr int CA_MAXDEV = 16;

// dynamic-LDS layout: d [2][dstride] floats | tok start, end [2][Lmax] ints | (route 1) back-pointer words [chunks][Smax]
struct CaLayout {
  int Smax, dstride, chunks;
  long base_bytes, bp_bytes;  // bp_bytes: per utterance
};
inline CaLayout ca_layout(int E, int Lmax) {
  CaLayout l;
  l.Smax = 2 * Lmax + 1;
  l.dstride = (l.Smax + 2 + 3) & ~3;
  l.chunks = (E + 15) / 16;
  l.base_bytes = ((2L * l.dstride + 2L * Lmax) * 4 + 15) & ~15L;
  l.bp_bytes = (long)l.chunks * l.Smax * 4;
  return l;
}

__device__ __forceinline__ float ca_lp(float v) { return v != v ? -__builtin_inff() : v; }  // a NaN counts as -inf

template <int PER, bool LDSBP>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ lp_all, long ld_b, long ld_t,
                                                        const int64_t* __restrict__ targets, int Lmax,
                                                        const int* __restrict__ in_lens, const int* __restrict__ tgt_lens,
                                                        int E, int V, int blank, int* frame_tok, int* __restrict__ tok_start,
                                                        int* __restrict__ tok_end, float* __restrict__ tok_score,
                                                        float* __restrict__ score, unsigned* bp_ws) {
  HIP_DYNAMIC_SHARED(float4, smem4)  // (float4: the base is 16-byte aligned)
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Smax = 2 * Lmax + 1, dstride = (Smax + 2 + 3) & ~3, chunks = (E + 15) / 16;
  float* dbuf = reinterpret_cast<float*>(smem4);
  int* ts = reinterpret_cast<int*>(dbuf + 2 * dstride);
  int* te = ts + Lmax;
  unsigned* bp = LDSBP ? reinterpret_cast<unsigned*>(reinterpret_cast<unsigned char*>(smem4) +
                                                     ((((long)2 * dstride + 2 * Lmax) * 4 + 15) & ~15L))
                       : bp_ws + (long)b * chunks * Smax;
  const int L = min(max(tgt_lens[b], 0), Lmax), Tb = min(max(in_lens[b], 0), E), S = 2 * L + 1;
  const float NEG = -__builtin_inff();
  const float* lp = lp_all + (long)b * ld_b;
  const int64_t* tg = targets + (long)b * Lmax;
  // label of target token i as a column of lp (an id outside [0, V) is clamped: no read leaves the row)
  auto column = [&](int i) { return (int)min(max(tg[i], (int64_t)0), (int64_t)(V - 1)); };

  // A thread's states: tid + 256 i, clamped to the last state -- a thread past the end repeats state S - 1 exactly (same
  // reads, same value, same addresses written), which keeps a frame free of branches: all its LDS reads issue together
  int sx[PER], col[PER];
  bool has2[PER];
  unsigned w[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int s = min(tid + 256 * i, S - 1);
    sx[i] = s;
    col[i] = (s & 1) ? column(s >> 1) : blank;
    has2[i] = (s & 1) && s >= 3 && column((s >> 1) - 1) != col[i];
    w[i] = 0u;
  }
  for (int i = tid; i < Lmax; i += 256) ts[i] = te[i] = -1;
  if (tid < 2) dbuf[tid] = dbuf[dstride + tid] = NEG;
  if (Tb > 0) {  // frame 0: states 0 and 1 are open
#pragma unroll
    for (int i = 0; i < PER; ++i) dbuf[2 + sx[i]] = sx[i] < 2 ? ca_lp(lp[col[i]]) : NEG;
  }
  // emissions: a ring of CA_DEPTH + 1 register slots.  The frame that consumes slot j fetches frame t + CA_DEPTH into the
  // slot the PREVIOUS frame consumed -- never into the one it is reading, so the compiler keeps every slot in its own
  // registers (no copies at the loop's back edge, which would wait for all outstanding loads).  The frame index is clamped
  // at the last frame: the loads are unconditional.
  float em[CA_DEPTH + 1][PER];
  const int tlast = max(Tb - 1, 0);
  if (Tb > 0) {
#pragma unroll
    for (int j = 0; j < CA_DEPTH; ++j)
#pragma unroll
      for (int i = 0; i < PER; ++i) em[j][i] = lp[(long)min(1 + j, tlast) * ld_t + col[i]];
  }
  __syncthreads();

  // one frame: emc holds its emissions; with `fetch`, emx receives those of frame t + CA_DEPTH
  auto step = [&](int t, const float (&emc)[PER], float (&emx)[PER], bool fetch) {
    if (fetch) {
      const long tn = min(t + CA_DEPTH, tlast);
#pragma unroll
      for (int i = 0; i < PER; ++i) emx[i] = lp[tn * ld_t + col[i]];
    }
    const float* pr = dbuf + ((t - 1) & 1) * dstride;
    float* cu = dbuf + (t & 1) * dstride;
    const int sh = 2 * (t & 15);
    float d0[PER], d1[PER], d2[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      d0[i] = pr[2 + sx[i]];
      d1[i] = pr[1 + sx[i]];
      d2[i] = pr[sx[i]];
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      float best = d0[i];
      unsigned k = 0u;
      if (d1[i] > best) { best = d1[i]; k = 1u; }           // ties go to the smaller jump: strict >
      if (has2[i] && d2[i] > best) { best = d2[i]; k = 2u; }
      cu[2 + sx[i]] = best + ca_lp(emc[i]);
      w[i] |= k << sh;
    }
    if ((t & 15) == 15 || t == Tb - 1) {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        bp[(long)(t >> 4) * Smax + sx[i]] = w[i];
        w[i] = 0u;
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): my LDS writes are done; global traffic stays in flight
    __builtin_amdgcn_s_barrier();
  };
  // straight-line over CA_DEPTH + 1 frames (a branch around a frame would make the compiler wait for ALL outstanding
  // loads where the paths join); the last <= CA_DEPTH frames run without fetching
  int t = 1;
  for (; t + CA_DEPTH + 1 <= Tb; t += CA_DEPTH + 1) {
#pragma unroll
    for (int j = 0; j <= CA_DEPTH; ++j) step(t + j, em[j], em[(j + CA_DEPTH) % (CA_DEPTH + 1)], true);
  }
#pragma unroll
  for (int j = 0; j < CA_DEPTH; ++j)
    if (t + j < Tb) step(t + j, em[j], em[j], false);  // (workgroup-uniform)
  __syncthreads();  // (route 2: the words other threads stored to the workspace are visible to the back-trace)

  // the path ends in state S - 1 only if that is strictly better than S - 2
  float sc = NEG;
  int end = 0;
  if (Tb > 0) {
    const float* last = dbuf + ((Tb - 1) & 1) * dstride;
    sc = last[2 + S - 1];
    end = S - 1;
    if (S > 1) {
      const float a = last[2 + S - 2];
      if (!(sc > a)) { sc = a; end = S - 2; }
    }
  }
  const bool feas = sc > NEG;  // (false for -inf and for a NaN that +inf inputs can make)
  int* ft = frame_tok + (long)b * E;
  if (tid == 0 && feas) {  // the back-trace: one lane, a dependent LDS (route 2: global) read whenever the state or chunk changes
    int s = end, ws = -1, wc = -1;
    unsigned word = 0u;
    for (int t = Tb - 1; t > 0; --t) {
      ft[t] = (s & 1) ? (s >> 1) : -1;
      const int c = t >> 4;
      if (c != wc || s != ws) { word = bp[(long)c * Smax + s]; wc = c; ws = s; }
      s -= (int)((word >> (2 * (t & 15))) & 3u);
    }
    ft[0] = (s & 1) ? (s >> 1) : -1;
  }
  __syncthreads();  // (frame_tok as lane 0 stored it is visible to the workgroup)
  if (feas) {       // token spans from the frame labels, one frame per thread: a token starts / ends where the label changes
    for (int t = tid; t < Tb; t += 256) {
      const int i = ft[t];
      if (i >= 0) {
        if (t == 0 || ft[t - 1] != i) ts[i] = t;
        if (t == Tb - 1 || ft[t + 1] != i) te[i] = t + 1;
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < E; t += 256)
    if (!feas || t >= Tb) ft[t] = -2;
  for (int i = tid; i < Lmax; i += 256) {
    int st = -1, en = -1;
    float q = 0.f;
    if (feas && i < L) {
      st = ts[i];
      en = te[i];
      const int c = column(i);
      float sum = 0.f;
      for (int t = st; t < en; ++t) sum += lp[(long)t * ld_t + c];  // in frame order
      q = sum / (float)(en - st);                                    // one IEEE division
    }
    tok_start[(long)b * Lmax + i] = st;
    tok_end[(long)b * Lmax + i] = en;
    tok_score[(long)b * Lmax + i] = q;
  }
  if (tid == 0) score[b] = feas ? sc : NEG;
}

// route 1 uses more than 64 KB of dynamic LDS: the attribute is set once per instantiation AND device
template <int PER>
bool ca_configure() {
  static bool done[CA_MAXDEV];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const bool cached = dev >= 0 && dev < CA_MAXDEV;
  if (cached && done[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_align_kernel<PER, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                          CA_LDS_MAX) != hipSuccess)
    return false;
  if (cached) done[dev] = true;
  return true;
}

}  // namespace

int64_t s2st_ctc_align_workspace(int32_t B, int32_t E, int32_t Lmax) {
  if (B <= 0 || E <= 0 || Lmax < 0) return 0;
  return (int64_t)B * ca_layout(E, Lmax).bp_bytes;
}

int s2st_ctc_align_f32(const float* lprobs, int64_t ld_b, int64_t ld_t, const int64_t* targets, int32_t Lmax,
                       const int32_t* in_lens, const int32_t* tgt_lens, int32_t B, int32_t E, int32_t V, int32_t blank,
                       int32_t route, int32_t* frame_tok, int32_t* tok_start, int32_t* tok_end, float* tok_score, float* score,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (B < 0 || E < 0 || Lmax < 0 || V < 1 || blank < 0 || blank >= V || route < 0 || route > 2) return S2ST_ERR_ARG;
  if (2L * Lmax + 1 > CA_MAXS) return S2ST_ERR_SHAPE;
  if (B == 0) return 0;
  if (!in_lens || !tgt_lens || !score || (E > 0 && (!lprobs || !frame_tok)) ||
      (Lmax > 0 && (!targets || !tok_start || !tok_end || !tok_score)))
    return S2ST_ERR_ARG;
  if (E > 0 && (ld_t < 0 || ld_b < 0)) return S2ST_ERR_ARG;
  const CaLayout l = ca_layout(E, Lmax);
  const bool fits = l.base_bytes + l.bp_bytes <= CA_LDS_MAX;
  if (route == 1 && !fits) return S2ST_ERR_SHAPE;
  const bool lds_bp = route == 1 || (route == 0 && fits);
  if (!lds_bp && l.bp_bytes > 0 && (!workspace || ((uintptr_t)workspace & 3) || workspace_bytes < (int64_t)B * l.bp_bytes))
    return S2ST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned lds = (unsigned)(l.base_bytes + (lds_bp ? l.bp_bytes : 0));
#define CA_LAUNCH(PER)                                                                                                       \
  do {                                                                                                                       \
    if (lds_bp) {                                                                                                            \
      if (!ca_configure<PER>()) return S2ST_ERR_LAUNCH;                                                                      \
      S2ST_LAUNCH((ctc_align_kernel<PER, true>), dim3(B), dim3(256), lds, st, lprobs, (long)ld_b, (long)ld_t, targets, Lmax, \
                  in_lens, tgt_lens, E, V, blank, frame_tok, tok_start, tok_end, tok_score, score, (unsigned*)nullptr);      \
    } else {                                                                                                                 \
      S2ST_LAUNCH((ctc_align_kernel<PER, false>), dim3(B), dim3(256), lds, st, lprobs, (long)ld_b, (long)ld_t, targets,      \
                  Lmax, in_lens, tgt_lens, E, V, blank, frame_tok, tok_start, tok_end, tok_score, score,                     \
                  (unsigned*)workspace);                                                                                     \
    }                                                                                                                        \
  } while (0)
  if (l.Smax <= 256) CA_LAUNCH(1);
  else if (l.Smax <= 512) CA_LAUNCH(2);
  else if (l.Smax <= 1024) CA_LAUNCH(4);
  else CA_LAUNCH(9);
#undef CA_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
