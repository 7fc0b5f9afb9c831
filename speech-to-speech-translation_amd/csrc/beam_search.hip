// Beam search over the aux ASR / ST text decoders' log-probabilities, on the device (include/s2st_hip.h s2st_beam_*).
//
// Reference call sites replaced: fairseq/sequence_generator.py:330-571 (the per-step masks, the EOS / finalise / active-
// hypothesis bookkeeping, the re-gather of the tokens / scores histories), fairseq/search.py:103-144 (BeamSearch.step:
// top 2 x beam of a sentence's beam x V candidate scores) and finalize_hypos (:607-716) up to the record of a finished
// hypothesis; the length normalisation, the differencing into positional scores and the final sort stay on the host
// (sequence_generator.py of this package), which reads the records once after the loop.
//
// One workgroup of 256 lanes per sentence.  Every lane scans a strided, coalesced slice of the candidates and keeps its own
// top K = 2 x beam in registers as 64-bit keys (order-preserving image of the fp32 score << 32 | ~flat index: the larger key
// is the better candidate, ties go to the smaller flat index -- the order a stable argsort of the negated scores yields,
// -inf ties included).  The workgroup's K winners are then taken in K rounds of an arg-max over the lanes' list heads (wave
// xor-shuffles, one LDS word per wave), and wave 0 does the bookkeeping of the K candidates with ballots and prefix counts.
#include <math.h>

#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_MAX_BEAM = 16;
constexpr int BS_HDR = 16;  // header words: 0 = finished sentences, 4 .. 8 = pad, unk, eos, min_len, unk_penalty

struct BeamLayout {  // offsets in 32-bit words
  long finished, n_final, ignore, final_step, final_score, final_tokens, final_scores, result_words, tokens, scores, total_words;
};
inline BeamLayout beam_layout(int bsz, int beam, int max_len) {
  const long R = (long)bsz * beam, L1 = max_len + 1;
  BeamLayout l;
  l.finished = BS_HDR;
  l.n_final = l.finished + bsz;
  l.ignore = l.n_final + bsz;
  l.final_step = l.ignore + R;
  l.final_score = l.final_step + R;
  l.final_tokens = l.final_score + R;
  l.final_scores = l.final_tokens + R * L1;
  l.result_words = l.final_scores + R * L1;
  l.tokens = l.result_words;
  l.scores = l.tokens + 2 * R * (L1 + 1);
  l.total_words = l.scores + 2 * R * L1;
  return l;
}

struct BeamConst {
  int pad, unk, eos, min_len, max_len;
  float unk_penalty;
};

// the masks of sequence_generator.py:152-159, in that order, then BeamSearch.step's add of the hypothesis' cumulative score
__device__ __forceinline__ float beam_candidate(float x, int v, int step, const BeamConst& c, float prev) {
  const float ninf = -INFINITY;
  if (step < c.min_len && v == c.eos) x = ninf;
  if (x != x) x = ninf;
  if (v == c.pad) x = ninf;
  if (v == c.unk) x = x - c.unk_penalty;
  if (step >= c.max_len && v != c.eos) x = ninf;
  if (step > 0) x = x + prev;
  return x;
}

// fp32 -> uint32 with the same order (-0 and +0 compare equal, as they do for the host's sort); every image is > 0
__device__ __forceinline__ uint32_t order_bits(float v) {
  const uint32_t u = (v == 0.f) ? 0u : __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int K>
struct TopK {  // descending; 0 = empty (below every key)
  unsigned long long a[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = 0ull;
  }
  __device__ __forceinline__ void push(unsigned long long x) {
    if (x > a[K - 1]) {
      a[K - 1] = x;
#pragma unroll
      for (int i = K - 1; i > 0; --i) {  // (static indices only: the list stays in registers)
        const unsigned long long hi = a[i] > a[i - 1] ? a[i] : a[i - 1], lo = a[i] > a[i - 1] ? a[i - 1] : a[i];
        a[i - 1] = hi;
        a[i] = lo;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int i = 0; i + 1 < K; ++i) a[i] = a[i + 1];
    a[K - 1] = 0ull;
  }
};

__global__ __launch_bounds__(BS_THREADS) void beam_begin_kernel(int* __restrict__ state, long tokens_off, long row_words, int R,
                                                                int pad, int unk, int eos, int min_len, float unk_penalty) {
  const int i = blockIdx.x * BS_THREADS + threadIdx.x;
  if (i < R) state[tokens_off + (long)i * row_words] = eos;  // tokens[:, 0] = eos (sequence_generator.py:137)
  if (i == 0) {
    state[4] = pad;
    state[5] = unk;
    state[6] = eos;
    state[7] = min_len;
    state[8] = __builtin_bit_cast(int, unk_penalty);
  }
}

template <int K>
__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(int* __restrict__ state, BeamLayout lay,
                                                               const float* __restrict__ lprobs, int V, int step, int beam,
                                                               int max_len, long long* __restrict__ tokens_next,
                                                               int* __restrict__ reorder) {
  __shared__ unsigned long long wave_best[2][BS_THREADS / 64];
  __shared__ unsigned long long winners[2 * BS_MAX_BEAM];
  __shared__ int rec_slot[BS_MAX_BEAM], rec_src[BS_MAX_BEAM], act_src[BS_MAX_BEAM], act_tok[BS_MAX_BEAM];
  __shared__ float rec_score[BS_MAX_BEAM], act_score[BS_MAX_BEAM];

  const int s = blockIdx.x, tid = threadIdx.x;
  const int L1 = max_len + 1, LT = max_len + 2, R = gridDim.x * beam;
  BeamConst c;
  c.pad = state[4];
  c.unk = state[5];
  c.eos = state[6];
  c.min_len = state[7];
  c.unk_penalty = __builtin_bit_cast(float, state[8]);
  c.max_len = max_len;
  const int cur = step & 1;
  const int* tok_cur = state + lay.tokens + (long)cur * R * LT;
  int* tok_new = state + lay.tokens + (long)(cur ^ 1) * R * LT;
  const float* sc_cur = (const float*)(state + lay.scores) + (long)cur * R * L1;
  float* sc_new = (float*)(state + lay.scores) + (long)(cur ^ 1) * R * L1;

  // ---- every lane's top K of its slice ---------------------------------------------------------------------------------
  const int nb = step == 0 ? 1 : beam;  // (step 0: every beam holds the same BOS prefix, only beam 0 is searched)
  const int cand = 2 * beam;
  const int k = min(cand, nb * V - 1);
  TopK<K> top;
  top.clear();
  for (int b = 0; b < nb; ++b) {
    const long row = (long)s * beam + b;
    const float prev = step > 0 ? sc_cur[row * L1 + step - 1] : 0.f;
    const float* lp = lprobs + row * V;
    const uint32_t base = 0xFFFFFFFFu - (uint32_t)(b * V);
    for (int v = tid; v < V; v += BS_THREADS) {
      const float x = beam_candidate(lp[v], v, step, c, prev);
      top.push(((unsigned long long)order_bits(x) << 32) | (unsigned long long)(base - (uint32_t)v));
    }
  }
  // ---- the workgroup's k best, in order ----------------------------------------------------------------------------------
  for (int r = 0; r < k; ++r) {
    unsigned long long m = top.a[0];
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const unsigned long long o = __shfl_xor(m, x);
      m = o > m ? o : m;
    }
    if ((tid & 63) == 0) wave_best[r & 1][tid >> 6] = m;
    __syncthreads();  // (one barrier per round: round r + 1 writes the other copy, round r + 2 comes after r + 1's barrier)
    const unsigned long long* wb = wave_best[r & 1];
    const unsigned long long b01 = wb[0] > wb[1] ? wb[0] : wb[1], b23 = wb[2] > wb[3] ? wb[2] : wb[3];
    const unsigned long long best = b01 > b23 ? b01 : b23;
    if (top.a[0] == best) top.pop();  // (keys are distinct: exactly one lane holds the winner)
    if (tid == 0) winners[r] = best;
  }
  __syncthreads();

  // ---- bookkeeping of the 2 x beam candidates: wave 0, lane = candidate rank --------------------------------------------------
  if (tid < 64) {
    const int r = tid;
    const bool valid = r < cand;
    float cs = -INFINITY;  // (ranks k .. 2 beam - 1 when the vocabulary is smaller than 2 x beam: dead entries)
    int cb = 0, ci = c.pad;
    if (r < k) {
      const uint32_t flat = 0xFFFFFFFFu - (uint32_t)winners[r];
      cb = (int)(flat / (uint32_t)V);
      ci = (int)(flat - (uint32_t)cb * (uint32_t)V);
      const long row = (long)s * beam + cb;
      cs = beam_candidate(lprobs[row * V + ci], ci, step, c, step > 0 ? sc_cur[row * L1 + step - 1] : 0.f);
    }
    const bool ign = r < beam && state[lay.ignore + (long)s * beam + r] != 0;
    const int fin0 = state[lay.finished + s], nf0 = state[lay.n_final + s];
    bool em = valid && ci == c.eos && cs != -INFINITY;
    if (ign || fin0) em = false;
    // finalize_hypos: the EOS candidates among the first `beam` ranks, in rank order, while the list is not full
    const bool sel = em && r < beam;
    const unsigned long long below = (1ull << r) - 1ull;
    const unsigned long long selm = __ballot(sel);
    const int nsel = __builtin_popcountll(selm);
    const int slot = nf0 + __builtin_popcountll(selm & below);
    if (r < beam) {
      rec_slot[r] = (sel && slot < beam) ? slot : -1;
      rec_src[r] = cb;
      rec_score[r] = cs;
    }
    const int nf1 = min(beam, nf0 + nsel);
    const int fin1 = (fin0 || (nsel > 0 && (nf1 == beam || step == max_len))) ? 1 : 0;
    // the hypotheses the next step continues: stable order of (masked, rank), first `beam`
    const bool masked = em || ign;
    const unsigned long long freem = __ballot(valid && !masked), maskm = __ballot(valid && masked);
    const int pos = !masked ? __builtin_popcountll(freem & below)
                            : __builtin_popcountll(freem) + __builtin_popcountll(maskm & below);
    if (valid && pos < beam) {  // (every lane read its old ignore flag before the ballots above)
      act_src[pos] = cb;
      act_tok[pos] = ci;
      act_score[pos] = cs;
      state[lay.ignore + (long)s * beam + pos] = masked ? 1 : 0;
    }
    if (r == 0) {
      state[lay.n_final + s] = nf1;
      state[lay.finished + s] = fin1;
      if (fin1 && !fin0) atomicAdd(&state[0], 1);
    }
  }
  __syncthreads();

  // ---- records of the hypotheses that ended here; histories of those that go on (all lanes) ---------------------------------
  int* fin_tok = state + lay.final_tokens;
  float* fin_sc = (float*)(state + lay.final_scores);
  for (int r = 0; r < beam; ++r) {
    const int slot = rec_slot[r];
    if (slot >= 0) {
      const long src = (long)s * beam + rec_src[r], dst = (long)s * beam + slot;
      const float es = rec_score[r];
      for (int j = tid; j <= step; j += BS_THREADS) {
        fin_tok[dst * L1 + j] = j < step ? tok_cur[src * LT + j + 1] : c.eos;
        fin_sc[dst * L1 + j] = j < step ? sc_cur[src * L1 + j] : es;
      }
      if (tid == 0) {
        state[lay.final_step + dst] = step;
        ((float*)state)[lay.final_score + dst] = es;
      }
    }
    const long src = (long)s * beam + act_src[r], dst = (long)s * beam + r;
    for (int j = tid; j <= step; j += BS_THREADS) {
      tok_new[dst * LT + j] = tok_cur[src * LT + j];
      if (j < step) sc_new[dst * L1 + j] = sc_cur[src * L1 + j];
    }
    if (tid == 0) {
      tok_new[dst * LT + step + 1] = act_tok[r];
      sc_new[dst * L1 + step] = act_score[r];
      tokens_next[dst] = (long long)act_tok[r];
      reorder[dst] = (int)src;
    }
  }
}

template <int K>
void launch_step(int* state, const BeamLayout& lay, const float* lprobs, int V, int step, int bsz, int beam, int max_len,
                 long long* tokens_next, int* reorder, hipStream_t st) {
  S2ST_LAUNCH(beam_step_kernel<K>, dim3((unsigned)bsz), dim3(BS_THREADS), 0, st, state, lay, lprobs, V, step, beam, max_len,
              tokens_next, reorder);
}

bool beam_shape_ok(int bsz, int beam, int max_len) { return bsz > 0 && beam >= 1 && beam <= BS_MAX_BEAM && max_len >= 0; }

}  // namespace

extern "C" {

int64_t s2st_beam_state_bytes(int32_t bsz, int32_t beam, int32_t max_len) {
  if (!beam_shape_ok(bsz, beam, max_len)) return S2ST_ERR_SHAPE;
  return 4 * (int64_t)beam_layout(bsz, beam, max_len).total_words;
}

int64_t s2st_beam_result_bytes(int32_t bsz, int32_t beam, int32_t max_len) {
  if (!beam_shape_ok(bsz, beam, max_len)) return S2ST_ERR_SHAPE;
  return 4 * (int64_t)beam_layout(bsz, beam, max_len).result_words;
}

int s2st_beam_begin(void* state, int32_t bsz, int32_t beam, int32_t max_len, int32_t pad, int32_t unk, int32_t eos,
                    int32_t min_len, float unk_penalty, void* stream) {
  if (!beam_shape_ok(bsz, beam, max_len)) return S2ST_ERR_SHAPE;
  if (!state) return S2ST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const BeamLayout lay = beam_layout(bsz, beam, max_len);
  if (hipMemsetAsync(state, 0, 4 * (size_t)lay.total_words, st) != hipSuccess) return S2ST_ERR_LAUNCH;
  const int R = bsz * beam;
  S2ST_LAUNCH(beam_begin_kernel, dim3((unsigned)((R + BS_THREADS - 1) / BS_THREADS)), dim3(BS_THREADS), 0, st, (int*)state,
              lay.tokens, (long)(max_len + 2), R, pad, unk, eos, min_len, unk_penalty);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_beam_step(void* state, int32_t bsz, int32_t beam, int32_t max_len, const float* lprobs, int32_t V, int32_t step,
                   int64_t* tokens_next_out, int32_t* reorder_out, void* stream) {
  if (!beam_shape_ok(bsz, beam, max_len) || V < 2 || (int64_t)beam * V >= (1ll << 31)) return S2ST_ERR_SHAPE;
  if (!state || !lprobs || !tokens_next_out || !reorder_out || step < 0 || step > max_len) return S2ST_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const BeamLayout lay = beam_layout(bsz, beam, max_len);
  int* s = (int*)state;
  long long* tn = (long long*)tokens_next_out;
  const int cand = 2 * beam;  // (the lanes' lists: the smallest instantiated size that holds 2 x beam entries)
  if (cand <= 2) launch_step<2>(s, lay, lprobs, V, step, bsz, beam, max_len, tn, reorder_out, st);
  else if (cand <= 4) launch_step<4>(s, lay, lprobs, V, step, bsz, beam, max_len, tn, reorder_out, st);
  else if (cand <= 10) launch_step<10>(s, lay, lprobs, V, step, bsz, beam, max_len, tn, reorder_out, st);
  else if (cand <= 16) launch_step<16>(s, lay, lprobs, V, step, bsz, beam, max_len, tn, reorder_out, st);
  else launch_step<32>(s, lay, lprobs, V, step, bsz, beam, max_len, tn, reorder_out, st);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_beam_fetch(const void* state, int32_t bsz, int32_t beam, int32_t max_len, void* host_out, void* stream) {
  if (!beam_shape_ok(bsz, beam, max_len)) return S2ST_ERR_SHAPE;
  if (!state || !host_out) return S2ST_ERR_ARG;
  const size_t n = 4 * (size_t)beam_layout(bsz, beam, max_len).result_words;
  return hipMemcpyAsync(host_out, state, n, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_beam_poll(const void* state, void* host_out_64_bytes, void* stream) {
  if (!state || !host_out_64_bytes) return S2ST_ERR_ARG;
  return hipMemcpyAsync(host_out_64_bytes, state, 4 * BS_HDR, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess
             ? 0 : S2ST_ERR_LAUNCH;
}

}  // extern "C"
