// engine_runtime.cpp -- per-call runtime: the second stream, bf16 casts, dropout seeds, parameter touches / overlapped
// optimizer waits, the queues of weight-gradient products and partial-sum folds, the weight-transpose tables.
#include <cstring>

#include "engine.h"
#include <hip/hip_ext.h>

using namespace s2st_eng;

// ------------------------------------------------------------------------------------
void s2st_engine::ensure_side() {        // the second stream and its events, on first need (the first training forward; the overlapped update)
  if (side_ || side_tried || !side_allowed) return;
  side_tried = true;
  // the side stream carries weight gradients nobody waits for until the segment ends: lowest queue priority, so that
  // when both queues have workgroups ready the data path (the critical chain of the backward) is dispatched first
  int pr_least = 0, pr_greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&pr_least, &pr_greatest) != hipSuccess) pr_least = 0;
  if (hipStreamCreateWithPriority(&side_, hipStreamNonBlocking, pr_least) != hipSuccess) side_ = nullptr;
  // No stream priorities: a plain second stream carries the same schedule.  This is also what gives the CPU emulator
  // (tests/hipemu: its priority form always fails) a second stream at all -- a label there, every launch is synchronous --
  // so the emulator suite now walks the second-stream schedule (aux heads, hoisted K|V projections, weight-gradient forks,
  // S2ST_DEC_OVERLAP) in its issue order instead of the one-stream one.
  if (!side_ && hipStreamCreateWithFlags(&side_, hipStreamNonBlocking) != hipSuccess) side_ = nullptr;
  bool ev_ok = side_ != nullptr;
  if (side_ && hipEventCreateWithFlags(&ev_kv_, hipEventDisableTiming) != hipSuccess) { ev_kv_ = nullptr; ev_ok = false; }
  if (side_ && hipEventCreateWithFlags(&ev_head_, hipEventDisableTiming) != hipSuccess) { ev_head_ = nullptr; ev_ok = false; }
  if (side_ && (hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_taps_, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&ev_auxb_, hipEventDisableTiming) != hipSuccess)) {
    hipStreamDestroy(side_);
    side_ = nullptr;
  }
  side_events_ = side_ && ev_ok;
}
hipStream_t s2st_engine::fork_side() {  // everything issued on st_ so far happens-before what follows on the returned stream
  if (!side_) return st_;
  hipEventRecord(ev_fork_, st_);
  hipStreamWaitEvent(side_, ev_fork_, 0);
  side_used = true;
  return side_;
}
void s2st_engine::wait_traced(hipStream_t st, hipEvent_t ev, const char* what) {
  if (!sw.stall_trace) { hipStreamWaitEvent(st, ev, 0); return; }
  Stall s{what, nullptr, nullptr};
  hipEventCreate(&s.a);
  hipEventCreate(&s.b);
  hipEventRecord(s.a, st);
  hipStreamWaitEvent(st, ev, 0);
  hipEventRecord(s.b, st);
  stalls.push_back(s);
}
void s2st_engine::join_side() {
  if (!side_ || !side_used) return;
  hipEventRecord(ev_join_, side_);
  wait_traced(st_, ev_join_, "join_side");
  side_used = false;
}

// bf16 copy of an activation / of its gradient (cast on first use unless the producer made it)
bf16raw* s2st_engine::half_of(Ten* t) {
  if (!t->h) {
    t->h = alloc_h((long)t->rows * t->hld());
    if (live()) chk(s2st_cast_bf16_rows(t->d, t->cols, t->h, t->hld(), t->rows, t->cols, st_));
  }
  return t->h;
}
bf16raw* s2st_engine::ghalf_of(Ten* t) {
  if (!t->gh) {
    t->gh = alloc_h((long)t->rows * t->hld());
    if (live()) chk(s2st_cast_bf16_rows(t->g, t->cols, t->gh, t->hld(), t->rows, t->cols, st_));
  }
  return t->gh;
}
bf16raw* s2st_engine::cast_buf(const float* x, long n) {  // whole-buffer twin (halo images, conv weights)
  bf16raw* y = alloc_h((n + 7) / 8 * 8);
  if (live()) chk(s2st_cast_bf16_rows(x, n, y, (n + 7) / 8 * 8, 1, (int)n, st_));
  return y;
}
// bf16 twin of a halo image [B][T + 2 pad][C] with zero halos; fast mode never reads the fp32 image's halos, so the
// callers do not clear it (alloc(n, !fast()))
// (plain: img is the plain rows [B * T][C] -- the first convolution of a stack needs no fp32 image at all)
bf16raw* s2st_engine::cast_halo(const float* img, int B, int T, int pad, int C, bool plain) {
  bf16raw* y = alloc_h(((long)B * (T + 2 * pad) * C + 7) / 8 * 8);
  if (live()) chk(s2st_cast_bf16_halo(img, y, B, T, pad, C, st_, plain ? 1 : 0));
  return y;
}
// the seed of the next dropout site (and, with the site log on, its record: engine.h)
uint64_t s2st_engine::next_seed(int kind, float p, long d0, long d1, long d2, long d3, long d4) {
  const uint64_t s = seed * 0x100000001B3ULL + (++site) * 0x9E3779B97F4A7C15ULL;
  if (site_log_on) {
    s2st_dropout_site r{};
    r.seed = s; r.kind = kind; r.p = p;
    r.dims[0] = d0; r.dims[1] = d1; r.dims[2] = d2; r.dims[3] = d3; r.dims[4] = d4;
    snprintf(r.ctx, sizeof r.ctx, "%s", site_ctx);
    int ord = 0;
    for (const s2st_dropout_site& q : site_log) ord += (q.kind == kind && !strcmp(q.ctx, r.ctx)) ? 1 : 0;
    r.ordinal = ord;
    site_log.push_back(r);
  }
  return s;
}
// ---- optimizer update overlapped with the next forward (s2st_engine_adam_overlapped) ------------------------------
// The fused scale / clip / Adam kernel runs in chunks of the arena on the SECOND stream, one event per chunk.  The
// arena is laid out in forward-use order and every op announces the parameters it is about to read (touch()), so the
// next forward on the data-path stream waits for exactly the chunks it needs, when it needs them; work the forward
// puts on the second stream (weight transposes, post-net weight layouts, hoisted K|V projections, aux heads) is
// ordered behind the update by the stream itself.
void s2st_engine::adam_wait_upto(long off_end) {
  if (!live()) return;
  while (adam_next < (int)adam_lo.size() && adam_lo[adam_next] < off_end) {
    hipStreamWaitEvent(st_, adam_ev[adam_next], 0);  // (st_ is the data-path stream here: touch() skips the second one)
    ++adam_next;
  }
  if (adam_next >= (int)adam_lo.size()) adam_pending = false;
}
int s2st_engine::adam_overlapped(float* m, float* v, const float* sumsq, int nparts, float gmul, const float* gmul_dev, float max_norm,
                    float lr, float b1, float b2, float eps, float wd, int step, float* gnorm_out, int* skipped, int use_ph,
                    int nchunks, hipStream_t main) {
  if (!P || !G || n_params <= 0) return S2ST_ERR_ARG;
  if (nchunks < 1) nchunks = 1;
  if (nchunks > 64) nchunks = 64;
  ensure_side();
  hipStream_t saved = st_;
  st_ = main;
  hipStream_t a = side_ ? fork_side() : main;  // behind the norm's partial sums (and everything else) on `main`
  st_ = saved;
  while ((int)adam_ev.size() < nchunks) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return S2ST_ERR_LAUNCH;
    adam_ev.push_back(e);
  }
  adam_lo.assign(nchunks, 0);
  int rc = 0;
  for (int c2 = 0; c2 < nchunks && !rc; ++c2) {
    const long lo = (n_params * c2 / nchunks) / 64 * 64, hi = c2 + 1 == nchunks ? n_params : (n_params * (c2 + 1) / nchunks) / 64 * 64;
    adam_lo[c2] = lo;
    // (every chunk folds the norm's partials itself; only the first one reports the norm and counts a skipped update)
    rc = s2st_adam(P + lo, G + lo, m + lo, v + lo, hi - lo, sumsq, gmul, gmul_dev, max_norm, lr, b1, b2, eps, wd, step,
                   c2 == 0 ? gnorm_out : nullptr, a, (use_ph && PH) ? reinterpret_cast<uint16_t*>(PH) + lo : nullptr,
                   c2 == 0 ? skipped : nullptr, nparts, 1);
    if (side_) hipEventRecord(adam_ev[c2], a);
  }
  adam_next = 0;
  adam_pending = side_ != nullptr && rc == 0;
  return rc;
}
// `stream` waits for the whole update (callers that read parameters outside the engine)
void s2st_engine::adam_wait_all(hipStream_t stream) {
  if (!adam_pending) return;
  for (int i = adam_next; i < (int)adam_lo.size(); ++i) hipStreamWaitEvent(stream, adam_ev[i], 0);
  adam_next = (int)adam_lo.size();
  adam_pending = false;
}

// ------------------------------------------------------------------------------------
// weight-gradient GEMMs waiting for their group launch (sw.group_wgrad, sw.group_flush_at)
void s2st_engine::push_wgrad(const GemmArgs& g) {
  for (const GemmArgs& p : pending_wgrad)
    if (p.C.p == g.C.p) { flush_wgrad(); break; }  // two sums into one matrix must not share a launch
  pending_wgrad.push_back(g);
  if ((int)pending_wgrad.size() >= sw.group_flush_at) flush_wgrad();
}
void s2st_engine::flush_wgrad() {
  if (pending_wgrad.empty()) return;
  if (live()) {
    // everything the products read was enqueued on st_ before this point
    hipStream_t s = (side_ && st_ != side_) ? fork_side() : st_;
    // S2ST_TIMING_SKIP_WGRAD=1 (-DS2ST_EXPERIMENTAL builds only: it makes the gradients WRONG): a timing experiment --
    // how much of the step is the weight-gradient products' share of the chip
#ifdef S2ST_EXPERIMENTAL
    static const bool skip = [] {
      const bool on = s2st_env_on("S2ST_TIMING_SKIP_WGRAD");
      if (on) fprintf(stderr, "[s2st] S2ST_TIMING_SKIP_WGRAD=1: weight-gradient products are SKIPPED -- gradients are WRONG, "
                              "timing experiments only\n");
      return on;
    }();
#else
    constexpr bool skip = false;
#endif
    if (!skip) chk(s2st_gemm_bf16_group(pending_wgrad.data(), (int)pending_wgrad.size(), s));
  }
  pending_wgrad.clear();
}

// the segment's batched fold of column-sum partials (pending_lnfold: engine.h)
void s2st_engine::flush_lnfold() {
  if (pending_lnfold.n == 0) return;
  if (live()) {
    hipStream_t s = (side_ && st_ != side_) ? fork_side() : st_;
    chk(s2st_layernorm_bwd_fold(pending_lnfold, s));
  }
  pending_lnfold = s2st_lnfold_table{};
}
// out[c] += sum_b part[b][c] (b in order) joins the segment's batched fold
void s2st_engine::add_fold(const float* part, int nblocks, int cols, float* out) {
  if (!part || nblocks <= 0 || cols <= 0) return;
  if (pending_lnfold.n == S2ST_LNFOLD_MAX) flush_lnfold();
  chk(s2st_fold_add(pending_lnfold, part, nblocks, cols, 1, out, nullptr, nullptr));
}

void s2st_engine::build_wt_tables() {
  s2st_transpose_table cur{};
  for (const WT& t : wt_list) {
    if (cur.n == S2ST_TRANSPOSE_MAX) { wt_tables.push_back(cur); cur = s2st_transpose_table{}; }
    const int i = cur.n++;
    cur.off[i] = (unsigned)t.off; cur.rows8[i] = (unsigned short)(t.N / 8); cur.cols8[i] = (unsigned short)(t.K / 8);
    cur.tile0[i + 1] = cur.tile0[i] + (unsigned)(((t.N + 63) / 64) * ((t.K + 63) / 64));
  }
  if (cur.n) wt_tables.push_back(cur);
}
