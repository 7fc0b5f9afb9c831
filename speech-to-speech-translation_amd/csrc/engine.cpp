// engine.cpp -- the extern "C" surface of the engine (include/s2st_hip.h: s2st_engine_*, s2st_hubert_*, s2st_w2v_ctc_*,
// s2st_hifigan_*) and the helpers only it uses.  The engine itself: engine.h and the engine_*.cpp units.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "engine.h"

using namespace s2st_eng;

namespace {
// The workspace a call needs: `body` runs in dry mode (sizes every allocation, launches nothing) on a workspace that is
// never dereferenced; the peak plus a margin, or the body's error.
template <class F>
int64_t dry_run_floats(s2st_engine* e, F body) {
  e->reset_call();
  e->dry = true;
  e->ws = reinterpret_cast<float*>(0x10000);
  e->ws_cap = (long)1 << 50;
  e->st_ = nullptr;
  const int rc = body();
  const long peak = e->ws_peak;
  e->reset_call();
  e->dry = false;
  return rc ? (int64_t)rc : (int64_t)peak + 1024;
}

// The forward-only aux decoder paths run on the call's stream alone: the second stream is hidden for the scope.
struct SingleStream {
  s2st_engine* e;
  hipStream_t side;
  explicit SingleStream(s2st_engine* e_) : e(e_), side(e_->side_) { e->side_ = nullptr; }
  ~SingleStream() { e->side_ = side; }
};

s2st_batch eval_batch(int B, int E, const int32_t* enc_lens) {
  s2st_batch b{};
  b.B = B; b.E = E; b.training = 0;
  b.enc_lens = enc_lens;
  return b;
}

bool aux_args_ok(const s2st_engine* e, int which) {
  return e && which >= 0 && which <= 1 && !((which == 0 && !e->c.has_asr) || (which == 1 && !e->c.has_st));
}

// The one place that reads the environment into the engine's table of switches (s2st_engine::Switches, where every field is
// documented).  Called once by each create path; a kind reads what it read before there was a table -- the rest of the
// table stays at its defaults.  (S2ST_DEC_OVERLAP is read per call by forward(); S2ST_CHAINS is checked by s2st_engine_create.)
void read_switches(s2st_engine::Switches& sw, s2st_engine::Kind kind) {
  // every kind
  sw.attn_keep_f32 = s2st_env_on("S2ST_ATTN_KEEP_F32");
  sw.convnet_fuse = s2st_env_int("S2ST_CONVNET_FUSE", 1) != 0;
  sw.use_streamk = s2st_env_on("S2ST_GEMM_STREAMK");
  if (kind == s2st_engine::Kind::HifiGan) return;
  // the transformer and the speech encoders
  sw.f32_operands = s2st_env_on("S2ST_F32_OPERANDS");
  sw.use_flash = !(s2st_env_on("S2ST_NO_FLASH"));
  if (kind == s2st_engine::Kind::SpeechEncoder) return;
  // the transformer
  sw.group_wgrad = !(s2st_env_on("S2ST_NO_WGRAD_GROUP"));
  if (s2st_env_str("S2ST_WGRAD_GROUP")) {
    sw.group_flush_at = atoi(s2st_env_str("S2ST_WGRAD_GROUP"));
    if (sw.group_flush_at < 1) sw.group_flush_at = 1;
    if (sw.group_flush_at > S2ST_GROUP_MAX) sw.group_flush_at = S2ST_GROUP_MAX;
  }
  sw.use_act_fuse = !(s2st_env_on("S2ST_NO_ACT_FUSE"));
  sw.use_only_h = !(s2st_env_on("S2ST_NO_ONLY_H"));
  sw.hoist_kv = !(s2st_env_on("S2ST_NO_KV_HOIST"));
  sw.stall_trace = s2st_env_on("S2ST_STALL_TRACE");
  sw.use_ln_skinny = !(s2st_env_on("S2ST_NO_LN_SKINNY"));
  sw.use_skinny = !(s2st_env_on("S2ST_NO_SKINNY"));
  sw.use_ln_fuse = !(s2st_env_on("S2ST_NO_LN_FUSE"));
  sw.attn_gfuse_mode = s2st_env_int("S2ST_ATTN_GFUSE", 1);
  sw.use_attn_gfuse = sw.attn_gfuse_mode != 0;
  sw.ln_bwd_split = s2st_env_on("S2ST_LN_BWD_SPLIT");
  sw.ordered_sums = !(s2st_env_int("S2ST_ORDERED_BIAS_SUMS", 1) == 0);
  sw.side_stream = !(s2st_env_on("S2ST_NO_SIDE_STREAM"));
  sw.overlap_aux = !(s2st_env_on("S2ST_NO_AUX_OVERLAP"));
}

// The two speech encoders' one create (engine_speech_encoder.cpp): cfg.vocab is read by the LayerNormPreLN variant only.
int speech_encoder_create(const s2st_w2v_ctc_config& cfg, s2st_engine::SpeechVariant v, s2st_engine** out) {
  const bool pre_ln = v == s2st_engine::SpeechVariant::LayerNormPreLN;
  if (cfg.n_conv < 1 || cfg.n_conv > 8 || (pre_ln && cfg.vocab < 1) || cfg.layers < 0 || cfg.heads < 1 ||
      cfg.conv_pos_groups < 1 || cfg.conv_pos < 1)
    return S2ST_ERR_ARG;
  if (cfg.embed % cfg.heads || cfg.embed % cfg.conv_pos_groups || (cfg.embed / cfg.conv_pos_groups) % 4 || cfg.embed % 4)
    return S2ST_ERR_SHAPE;
  for (int i = 0; i < cfg.n_conv; ++i)
    if (cfg.conv_k[i] < 1 || cfg.conv_stride[i] < 1) return S2ST_ERR_SHAPE;
  // what the variant's kernels take: conv 0 (s2st_hubert_conv0_gn_gelu / s2st_w2v_conv0_ln_gelu) and, LayerNormPreLN, the
  // row kernel behind every later convolution (s2st_w2v_ln_gelu_rows)
  if (!pre_ln && cfg.conv_dim[0] % 4) return S2ST_ERR_SHAPE;
  if (pre_ln && (cfg.conv_dim[0] > 512 || cfg.conv_k[0] > 16)) return S2ST_ERR_SHAPE;
  for (int i = 0; pre_ln && i < cfg.n_conv; ++i)
    if (cfg.conv_dim[i] < 4 || cfg.conv_dim[i] % 4 || cfg.conv_dim[i] > 1024) return S2ST_ERR_SHAPE;
  if (!cfg.precise) {
    for (int i = 0; i < cfg.n_conv; ++i)
      if (cfg.conv_dim[i] % 8) return S2ST_ERR_SHAPE;
    if (cfg.embed % 8 || cfg.ffn % 8 || (cfg.embed / cfg.conv_pos_groups) % 8) return S2ST_ERR_SHAPE;
  }
  s2st_engine* e = new s2st_engine();
  e->kind = s2st_engine::Kind::SpeechEncoder;
  e->sv = v;
  e->sc = cfg;
  e->c = s2st_model_config{};
  e->c.precise = cfg.precise;
  e->c.enc_heads = cfg.heads;
  e->c.enc_dim = cfg.embed;
  e->ffn_act = 2;
  read_switches(e->sw, e->kind);
  // the recogniser: every product goes through the tiled GEMM whatever the batch's row count: an utterance's logits do not
  // depend on what else is in the batch
  if (pre_ln) e->sw.use_skinny = false;
  e->build_params_speech();
  // (a process that replays HIP graphs can carry a stale "last error" of the runtime's own capture-time queries: the preload's
  //  launch checks must see their own errors only)
  (void)hipGetLastError();
  if (!cfg.precise && (s2st_gemm_bf16_preload(nullptr) != 0 || s2st_flash_attn_preload(nullptr) != 0)) { delete e; return S2ST_ERR_LAUNCH; }
  *out = e;
  return 0;
}
}  // namespace

// ---------------------------------------------------------------------------------------------
extern "C" {

int s2st_engine_create(const s2st_model_config* cfg, s2st_engine** out) {
  if (!cfg || !out) return S2ST_ERR_ARG;
  if (cfg->enc_dim % cfg->enc_heads || cfg->dec_dim % cfg->dec_heads || cfg->enc_dim % 4 ||
      cfg->dec_dim % 4 || cfg->in_dim % 4 || cfg->out_dim % 4 || cfg->conv_channels % 8)
    return S2ST_ERR_SHAPE;
  // bf16-operand mode reads 16-byte chunks of 8 elements: every projection width must be % 8
  if (!cfg->precise && (cfg->enc_dim % 8 || cfg->dec_dim % 8 || cfg->in_dim % 8 || cfg->out_dim % 8 ||
                        cfg->prenet_dim % 8 || cfg->postnet_dim % 8 || cfg->enc_ffn % 8 || cfg->dec_ffn % 8 ||
                        cfg->conv_channels % 16 || (cfg->has_asr && cfg->asr_dim % 8) ||
                        (cfg->has_st && cfg->st_dim % 8)))
    return S2ST_ERR_SHAPE;
  // the two-utterance-half-chain schedule measured neutral and was removed (profiles/r05_chains_ab.txt): asked for and not available is loud
  if (!cfg->precise && s2st_env_int("S2ST_CHAINS", 1) != 1) return S2ST_ERR_ARG;
  // guided-attention term: a mel decoder's alignment layer and a positive sigma
  if (cfg->guided && (cfg->s2t_mode || cfg->dec_layers <= 0 || !(cfg->guided_sigma > 0.f))) return S2ST_ERR_ARG;
  s2st_engine* e = new s2st_engine();
  e->c = *cfg;
  read_switches(e->sw, e->kind);
  e->build_params();
  // (a process that replays HIP graphs can carry a stale "last error" of the runtime's own capture-time queries: the preload's
  //  launch checks must see their own errors only)
  (void)hipGetLastError();
  if (!cfg->precise && (s2st_gemm_bf16_preload(nullptr) != 0 || s2st_flash_attn_preload(nullptr) != 0)) { delete e; return S2ST_ERR_LAUNCH; }
  // The second stream is made at the first TRAINING forward (ensure_side), not here: a process has four hardware queues
  // (runtime/streams.py) and an engine that only ever decodes would hold one of them for nothing -- the caller's stream
  // then shares a queue with one of the generator's chains (config 5, profiles/r05_queue_matrix.txt).
  e->side_allowed = !cfg->precise && e->sw.side_stream;
  *out = e;
  return 0;
}

void s2st_engine_destroy(s2st_engine* e) {
  if (!e) return;
  if (e->side_) {
    hipStreamSynchronize(e->side_);
    hipStreamDestroy(e->side_);
    hipEventDestroy(e->ev_fork_);
    hipEventDestroy(e->ev_join_);
    if (e->ev_taps_) hipEventDestroy(e->ev_taps_);
    if (e->ev_auxb_) hipEventDestroy(e->ev_auxb_);
    if (e->ev_kv_) hipEventDestroy(e->ev_kv_);
    if (e->ev_head_) hipEventDestroy(e->ev_head_);
    for (hipEvent_t ev : e->adam_ev) hipEventDestroy(ev);
  }
  e->reset_call();
  delete e;
}

int32_t s2st_engine_num_params(const s2st_engine* e) { return (int32_t)e->infos.size(); }

int s2st_engine_param_info(const s2st_engine* e, int32_t i, s2st_param_info* out) {
  if (i < 0 || i >= (int)e->infos.size()) return S2ST_ERR_ARG;
  const PInfo& p = e->infos[i];
  memset(out, 0, sizeof(*out));
  strncpy(out->name, p.name.c_str(), sizeof(out->name) - 1);
  out->offset = p.off;
  out->numel = p.numel;
  out->ndim = p.ndim;
  for (int k = 0; k < 4; ++k) out->shape[k] = p.shape[k];
  out->is_buffer = p.is_buffer;
  return 0;
}

int64_t s2st_engine_param_floats(const s2st_engine* e) { return e->n_params; }
int64_t s2st_engine_buffer_floats(const s2st_engine* e) { return e->n_buffers; }

int s2st_engine_bind(s2st_engine* e, float* params, float* grads, float* buffers) {
  e->P = params;
  e->G = grads;
  e->BUF = buffers;
  return 0;
}

int s2st_engine_bind_bf16(s2st_engine* e, uint16_t* params_bf16) {
  e->PH = params_bf16;
  return 0;
}

// allow = 0: this engine never makes (or sizes scratch for) a second stream -- inference twins, which only ever decode
// (a stream created all the same would take a hardware-queue slot: runtime/streams.py).  Call before the first forward.
int s2st_engine_allow_side_stream(s2st_engine* e, int32_t allow) {
  if (!e) return S2ST_ERR_ARG;
  if (e->side_) return allow ? S2ST_OK : S2ST_ERR_ARG;  // (already made: cannot be taken back)
  e->side_allowed = allow != 0 && !e->c.precise;
  return S2ST_OK;
}

// Dropout-site log (test instrumentation, see Engine::next_seed): on = 1 makes every later forward record its sites;
// s2st_engine_site_log_get copies the records of the LAST forward (at most cap) and returns their number.
int s2st_engine_site_log(s2st_engine* e, int32_t on) {
  if (!e) return S2ST_ERR_ARG;
  e->site_log_on = on != 0;
  if (!on) e->site_log.clear();
  return S2ST_OK;
}
int32_t s2st_engine_site_log_get(const s2st_engine* e, s2st_dropout_site* out, int32_t cap) {
  if (!e) return -1;
  const int32_t n = (int32_t)e->site_log.size();
  for (int32_t i = 0; i < n && i < cap && out; ++i) out[i] = e->site_log[i];
  return n;
}

// S2ST_STALL_TRACE=1: prints (stderr) and clears the cross-stream waits recorded since the last report; the caller
// has synchronised the device.  Returns the total wait in microseconds.
int64_t s2st_engine_stall_report(s2st_engine* e, int32_t verbose) {
  if (!e) return S2ST_ERR_ARG;
  double total = 0;
  for (auto& s : e->stalls) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      total += ms * 1e3;
      if (verbose) fprintf(stderr, "[stall] %-44s %8.1f us\n", s.what, ms * 1e3);
    }
    hipEventDestroy(s.a);
    hipEventDestroy(s.b);
  }
  e->stalls.clear();
  return (int64_t)total;
}

int s2st_engine_bf16_is_fresh(s2st_engine* e) {
  if (!e || !e->PH) return S2ST_ERR_ARG;
  e->ph_fresh = true;
  return 0;
}

int s2st_engine_bind_bf16_transposed(s2st_engine* e, uint16_t* params_bf16_t) {
  e->PHT = params_bf16_t;
  return 0;
}

int64_t s2st_engine_workspace_floats(s2st_engine* e, const s2st_batch* b) {
  return dry_run_floats(e, [&] {
    e->bt = *b;
    memset(&e->outs, 0, sizeof(e->outs));  // outputs the caller may keep internal are counted as workspace
    int rc = e->forward();
    if (rc == 0) {
      e->gscale = 1.f;
      for (int s = 0; s < e->n_segments(); ++s) e->backward_segment(s);
    }
    return rc;
  });
}

int s2st_engine_forward(s2st_engine* e, const s2st_batch* b, const s2st_outputs* out, float* workspace,
                        int64_t workspace_floats, void* stream) {
  if (!e->P || !e->BUF) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt = *b;
  e->outs = *out;
  if (!e->outs.stats && b->tgt) return S2ST_ERR_ARG;
  return e->forward();  // (the tape stays for the backward)
}

int s2st_engine_backward(s2st_engine* e, float gscale, int32_t segment, void* stream) {
  if (!e->G) return S2ST_ERR_ARG;
  e->st_ = (hipStream_t)stream;
  e->gscale = gscale;
  if (segment < 0) {
    for (int s = 0; s < e->n_segments(); ++s) {
      int rc = e->backward_segment(s);
      if (rc) return rc;
    }
    return 0;
  }
  return e->backward_segment(segment);
}

int s2st_engine_adam_overlapped(s2st_engine* e, float* exp_avg, float* exp_avg_sq, const float* sumsq_parts, int32_t n_parts,
                                float gmul, const float* gmul_dev, float max_norm, float lr, float beta1, float beta2, float eps,
                                float wd, int32_t step, float* gnorm_out, int32_t* skipped, int32_t write_bf16, int32_t n_chunks,
                                void* stream) {
  if (!e || !exp_avg || !exp_avg_sq || !sumsq_parts || n_parts <= 0) return S2ST_ERR_ARG;
  return e->adam_overlapped(exp_avg, exp_avg_sq, sumsq_parts, n_parts, gmul, gmul_dev, max_norm, lr, beta1, beta2, eps, wd, step,
                            gnorm_out, skipped, write_bf16, n_chunks, (hipStream_t)stream);
}

int s2st_engine_wait_optimizer(s2st_engine* e, void* stream) {
  if (!e) return S2ST_ERR_ARG;
  e->adam_wait_all((hipStream_t)stream);
  return 0;
}

int32_t s2st_engine_num_segments(const s2st_engine* e) { return e->n_segments(); }

int32_t s2st_engine_dec_overlap_active(const s2st_engine* e) {
  return e ? (e->dec_early_active ? 1 : 0) | (e->tail_bwd_on_side ? 2 : 0) : 0;
}

void* s2st_engine_side_stream(const s2st_engine* e) {  // (a trainer asks before the first forward: made on demand)
  const_cast<s2st_engine*>(e)->ensure_side();
  return (void*)e->side_;
}

int s2st_engine_segment_range(const s2st_engine* e, int32_t i, int64_t* lo, int64_t* hi) {
  int ns = e->n_segments();
  if (i < 0 || i >= ns) return S2ST_ERR_ARG;
  *lo = e->marks[ns - i - 1].param_off;
  *hi = e->marks[ns - i].param_off;
  return 0;
}

// ---- AR decoding + eval post-net (config 5) ---------------------------------------------------
int64_t s2st_engine_decode_state_floats(const s2st_engine* e, int32_t B, int32_t E, int32_t max_steps) {
  const long Cd = e->c.dec_dim, L = e->c.dec_layers;
  // self-attention caches | static cross-attention keys and values | pad | alpha-scaled position rows | bf16 copies of the
  // cross-attention rows (fast mode)
  return L * 2 * B * (long)max_steps * Cd + L * (long)B * E * 2 * Cd + 64 + ((long)max_steps + 2) * Cd + L * (long)B * E * Cd + 8;
}

int s2st_engine_decode_begin(s2st_engine* e, const s2st_batch* b, const s2st_outputs* out, float* state,
                             int64_t state_floats, int32_t max_steps, float* workspace, int64_t workspace_floats,
                             void* stream) {
  if (!e->P || !e->BUF || !state || !b || !out) return S2ST_ERR_ARG;
  if (state_floats < s2st_engine_decode_state_floats(e, b->B, b->E, max_steps)) return S2ST_ERR_WORKSPACE;
  e->dec_row_map = nullptr;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt = *b;
  e->bt.training = 0;
  e->bt.tgt = nullptr;
  e->outs = *out;
  e->stop_after_encoder = true;
  e->adam_wait_all((hipStream_t)stream);  // (the AR steps read every decoder parameter; not left to the per-chunk waits of a forward that stops early)
  int rc = e->forward();
  e->stop_after_encoder = false;
  if (rc) return rc;
  e->dec_st.base = state;
  e->dec_st.B = b->B; e->dec_st.E = b->E; e->dec_st.maxT = max_steps;
  e->dec_st.enc_lens = b->enc_lens;
  e->dec_st.pe_dec = b->pe_dec;
  // alpha-scaled position rows 0 .. max_steps + 1 (one small launch per utterance batch instead of one per step)
  {
    const long Cd = e->c.dec_dim, L = e->c.dec_layers;
    e->dec_st.pe_alpha = state + L * 2 * b->B * (long)max_steps * Cd + L * (long)b->B * b->E * 2 * Cd + 64;
    e->touch(e->pos_alpha + 1);
    if (e->live())
      e->chk(s2st_scale_rows(b->pe_dec, e->P + e->pos_alpha, e->dec_st.pe_alpha, ((long)max_steps + 2) * Cd, e->st_));
  }
  // static cross-attention keys / values of every decoder layer (static_kv=True)
  // (bf16 copies of the static rows for the decode steps' cross-attention were built in round 4 and measured SLOWER than the
  //  fp32 rows -- 15.0 against 13.3 us per launch, profiles/r04_t_decode_attn_bench.txt; the kernel form stays in the C ABI
  //  (s2st_decode_attn, kv_bf16), the engine switch is gone)
  for (int l = 0; l < e->c.dec_layers; ++l) {
    const XAttnP& xa = e->dec[l].xa;
    e->linear(e->enc_out_keep, xa.kv_w, xa.kv_b, 2 * e->c.dec_dim, e->c.enc_dim, 0, 0.f, nullptr, e->dec_crossKV(l));
  }
  return e->end_call(0);
}

// Several batches decoded as ONE (round 6): the always-on Prenet dropout (tacotron2.py:95-98) keys its mask by the row of the
// batch, so the rows of the 2nd, 3rd ... batch say which row of their own batch they are.  NULL: rows count from 0.
// Set after decode_begin (which clears it), holds for the run's steps; the non-skinny paths (more than 256 rows) ignore it.
int s2st_engine_decode_row_map(s2st_engine* e, const int32_t* row_map) {
  if (!e) return S2ST_ERR_ARG;
  e->dec_row_map = row_map;
  return S2ST_OK;
}

int s2st_engine_decode_step(s2st_engine* e, int32_t step, const float* prev, const int32_t* pos,
                            const int32_t* self_klen, uint64_t seed, float* feat_out, float* eos_prob,
                            float* attn_out, float* workspace, int64_t workspace_floats, void* stream) {
  if (!e->P || !prev || !pos || !feat_out || !eos_prob) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  if (int rc = e->params_ready(false, false)) return rc;  // PH was refreshed by decode_begin's forward
  return e->end_call(e->decode_step(step, prev, pos, self_klen, seed, feat_out, eos_prob, attn_out));
}

// ---- the decode step in its graph-replayable form (include/s2st_hip.h: s2st_decode_replay) --------------------------------
// 1 when the run decode_begin prepared is made of the forms decode_step_replay can take (bf16-operand mode, skinny products
// for <= 64 utterances, the position row and the logistic fused): the conditions decode_step itself checks, asked up front
int32_t s2st_engine_decode_replay_supported(const s2st_engine* e) {
  if (!e || !e->dec_st.base || !e->dec_st.pe_alpha || !e->fast() || !e->PH || !e->sw.use_skinny) return 0;
  const int B = e->dec_st.B, Cd = e->c.dec_dim;
  if (B < 1 || B > 64 || e->c.prenet_dim % 32 || e->c.out_dim % 32 || Cd % 64 || e->c.prenet_layers > 7) return 0;
  if (e->has_dec_ln && !e->sw.use_ln_skinny) return 0;
  return 1;
}

int s2st_engine_decode_replay_begin(s2st_engine* e, const s2st_decode_replay* r, uint64_t seed0, void* stream) {
  if (!e || !r || !e->dec_st.base || !e->dec_st.pe_alpha) return S2ST_ERR_ARG;
  return s2st_decode_replay_init(r->step, r->seeds, r->cur_feat, (long)e->dec_st.B * e->c.out_dim, r->pe_cur, e->dec_st.pe_alpha,
                                 e->c.dec_dim, seed0, (hipStream_t)stream);
}

int s2st_engine_decode_step_replay(s2st_engine* e, const s2st_decode_replay* r, const int32_t* self_klen, float* workspace,
                                   int64_t workspace_floats, void* stream) {
  if (!e || !e->P || !r || !r->step || !r->seeds || !r->cur_feat || !r->cur_eos || !r->pe_cur) return S2ST_ERR_ARG;
  if (!e->fast() || !e->PH || !e->dec_st.pe_alpha) return S2ST_ERR_SHAPE;
  e->begin_call(workspace, workspace_floats, stream);
  if (int rc = e->params_ready(false, false)) return rc;
  e->replay_ = r;
  // (step 0 / seed 0 on the host side: every step-dependent value comes from *r inside the kernels)
  int rc = e->decode_step(0, r->cur_feat, nullptr, self_klen, 0, r->cur_feat, r->cur_eos, r->cur_attn);
  e->replay_ = nullptr;
  return e->end_call(rc);
}

int s2st_engine_decode_replay_commit(s2st_engine* e, const s2st_decode_replay* r, uint64_t seed0, float thr, int32_t max_iter,
                                     int32_t* finished, int32_t* out_lens, int32_t* klen_next, int32_t* n_done,
                                     float* feat_all, float* eos_all, float* attn_all, void* stream) {
  if (!e || !r || !e->dec_st.base || !e->dec_st.pe_alpha) return S2ST_ERR_ARG;
  return s2st_decode_replay_commit(r->step, r->seeds, r->cur_feat, r->cur_eos, r->cur_attn, r->pe_cur, e->dec_st.pe_alpha,
                                   e->dec_st.maxT + 2, e->c.dec_dim, seed0, thr, max_iter, e->dec_st.B, e->c.out_dim, e->dec_st.E,
                                   finished, out_lens, klen_next, n_done, feat_all, eos_all, attn_all, (hipStream_t)stream);
}

int s2st_engine_postnet_eval(s2st_engine* e, const float* feat, int32_t B, int32_t D, float* post_out,
                             float* workspace, int64_t workspace_floats, void* stream) {
  if (!e->P || !e->BUF || !feat || !post_out) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt.training = 0;
  if (int rc = e->params_ready()) return rc;
  std::vector<s2st_engine::ConvW> csp;
  for (auto& pc : e->post_conv) csp.push_back(e->make_conv_scratch(pc, false, false));
  Ten* f = e->newT(B * D, e->c.out_dim, const_cast<float*>(feat));
  f->needs_grad = false;
  e->postnet(f, B, D, false, csp, post_out);
  return e->end_call(0);
}

// ---- aux ASR / ST text decoder, forward only (beam search over an aux head: generate_for_s2st.py:107-111) -----
int s2st_engine_aux_decode(s2st_engine* e, int32_t which, const float* tap, const int32_t* enc_lens,
                           const int64_t* prev_tokens, const int32_t* positions, const int32_t* lens, const float* pe,
                           int32_t Bb, int32_t L, int32_t E, float* logits_out, float* workspace,
                           int64_t workspace_floats, void* stream) {
  if (!aux_args_ok(e, which) || !e->P || !tap || !enc_lens || !prev_tokens || !positions || !lens || !pe || !logits_out)
    return S2ST_ERR_ARG;
  if (Bb <= 0 || L <= 0 || E <= 0) return S2ST_ERR_SHAPE;
  if (!workspace) return S2ST_ERR_WORKSPACE;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt = eval_batch(Bb, E, enc_lens);
  if (int rc = e->params_ready()) return rc;
  SingleStream one(e);
  Ten* t = e->newT(Bb * E, e->c.enc_dim, const_cast<float*>(tap));
  t->needs_grad = false;
  e->aux_decoder(which == 0 ? e->asr : e->st, t, (const long*)prev_tokens, positions, lens, Bb, L, pe, logits_out);
  return e->end_call(0);
}

// ---- the same decoder step by step with key / value caches (include/s2st_hip.h) --------------------------------------------
int64_t s2st_engine_aux_inc_state_floats(const s2st_engine* e, int32_t which, int32_t Bb, int32_t E, int32_t max_len) {
  if (!aux_args_ok(e, which) || Bb <= 0 || E <= 0 || max_len <= 0) return S2ST_ERR_ARG;
  const AuxP& a = which == 0 ? e->asr : e->st;
  return 2 * s2st_engine::aux_inc_half(a, Bb, max_len) + (long)a.layers * Bb * E * 2 * a.d + 64;
}

int64_t s2st_engine_aux_inc_workspace(const s2st_engine* e, int32_t which, int32_t Bb, int32_t E) {
  if (!aux_args_ok(e, which) || Bb <= 0 || E <= 0) return S2ST_ERR_ARG;
  const AuxP& a = which == 0 ? e->asr : e->st;
  // begin: bf16 copies of the tap and of every layer's K | V projection; a step: a few dozen [Bb][width] tensors
  long w = a.in_dim;
  for (long v : {(long)3 * a.d, (long)e->c.dec_ffn, (long)a.V, (long)a.out_dim, (long)e->c.enc_dim}) w = v > w ? v : w;
  return (long)Bb * E * (e->c.enc_dim + 2L * a.layers * a.d) + 96L * Bb * w + (1L << 20);
}

int s2st_engine_aux_inc_begin(s2st_engine* e, int32_t which, const float* tap, const int32_t* enc_lens, int32_t Bb, int32_t E,
                              int32_t max_len, float* state, float* workspace, int64_t workspace_floats, void* stream) {
  if (!aux_args_ok(e, which) || !e->P || !tap || !enc_lens || !state) return S2ST_ERR_ARG;
  if (Bb <= 0 || E <= 0 || max_len <= 0) return S2ST_ERR_SHAPE;
  if (!workspace) return S2ST_ERR_WORKSPACE;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt = eval_batch(Bb, E, enc_lens);
  if (int rc = e->params_ready()) return rc;
  SingleStream one(e);
  s2st_engine::AuxInc& S = e->aux_inc[which];
  S = s2st_engine::AuxInc{};
  S.base = state; S.Bb = Bb; S.E = E; S.maxT = max_len; S.enc_lens = enc_lens;
  Ten* t = e->newT(Bb * E, e->c.enc_dim, const_cast<float*>(tap));
  t->needs_grad = false;
  return e->end_call(e->aux_inc_begin(which == 0 ? e->asr : e->st, S, t));
}

int s2st_engine_aux_inc_step(s2st_engine* e, int32_t which, int32_t step, const int64_t* tokens, const int32_t* reorder,
                             const int32_t* positions, const float* pe, float* logits_out, float* workspace,
                             int64_t workspace_floats, void* stream) {
  if (!aux_args_ok(e, which) || !e->P || !tokens || !positions || !pe || !logits_out) return S2ST_ERR_ARG;
  if (!workspace) return S2ST_ERR_WORKSPACE;
  s2st_engine::AuxInc& S = e->aux_inc[which];
  if (!S.base) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  e->bt = eval_batch(S.Bb, S.E, S.enc_lens);
  if (int rc = e->params_ready(false, false)) return rc;  // (PH was refreshed by aux_inc_begin)
  SingleStream one(e);
  return e->end_call(e->aux_inc_step(which == 0 ? e->asr : e->st, S, step, (const long*)tokens, reorder, positions, pe,
                                     logits_out));
}

int64_t s2st_engine_aux_decode_workspace(s2st_engine* e, int32_t which, int32_t Bb, int32_t L, int32_t E) {
  if (!aux_args_ok(e, which)) return S2ST_ERR_ARG;
  return dry_run_floats(e, [&] {
    e->bt = eval_batch(Bb, E, nullptr);
    SingleStream one(e);
    Ten* t = e->newT(Bb * E, e->c.enc_dim, e->ws);  // (tap and logits: the dry workspace, never dereferenced)
    t->needs_grad = false;
    e->aux_decoder(which == 0 ? e->asr : e->st, t, nullptr, nullptr, nullptr, Bb, L, nullptr, e->ws);
    return e->err;
  });
}

// ---- the speech encoders: HuBERT front end, wav2vec 2.0 CTC recogniser -----------------------------
int s2st_hubert_create(const s2st_hubert_config* cfg, s2st_engine** out) {
  if (!cfg || !out) return S2ST_ERR_ARG;
  static_assert(offsetof(s2st_w2v_ctc_config, vocab) == sizeof(s2st_hubert_config), "s2st_hubert_config is the prefix");
  s2st_w2v_ctc_config full{};
  memcpy(&full, cfg, sizeof(*cfg));
  return speech_encoder_create(full, s2st_engine::SpeechVariant::GroupNormPostLN, out);
}

int32_t s2st_hubert_out_frames(const s2st_engine* e, int32_t n_samples) { return e->speech_frames(n_samples); }

int64_t s2st_hubert_workspace_floats(s2st_engine* e, int32_t B, int32_t N) {
  if (!e->is_speech(s2st_engine::SpeechVariant::GroupNormPostLN)) return S2ST_ERR_ARG;
  return dry_run_floats(e, [&] { return e->forward_speech(nullptr, nullptr, nullptr, B, N, nullptr, 0, nullptr, nullptr); });
}

int s2st_hubert_forward(s2st_engine* e, const float* wave, const int32_t* frame_lens, int32_t B, int32_t N, float* out,
                        float* workspace, int64_t workspace_floats, void* stream) {
  if (!e->is_speech(s2st_engine::SpeechVariant::GroupNormPostLN) || !e->P || !wave || !frame_lens || !out) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  // frozen weights: the host side tracks the parameter tensor's version and vouches for the bf16 copy (0.1 ms of the
  // 6.9 ms forward); forward only: the front end is frozen (s2st_transformer.py:245-249)
  if (int rc = e->params_ready()) return rc;
  return e->end_call(e->forward_speech(wave, nullptr, frame_lens, B, N, out, 0, nullptr, nullptr));
}

int s2st_w2v_ctc_create(const s2st_w2v_ctc_config* cfg, s2st_engine** out) {
  if (!cfg || !out) return S2ST_ERR_ARG;
  return speech_encoder_create(*cfg, s2st_engine::SpeechVariant::LayerNormPreLN, out);
}

int32_t s2st_w2v_ctc_out_frames(const s2st_engine* e, int32_t n_samples) {
  if (!e || !e->is_speech(s2st_engine::SpeechVariant::LayerNormPreLN)) return S2ST_ERR_ARG;
  return e->speech_frames(n_samples);
}

int64_t s2st_w2v_ctc_workspace_floats(s2st_engine* e, int32_t B, int32_t N) {
  if (!e || !e->is_speech(s2st_engine::SpeechVariant::LayerNormPreLN) || B <= 0 || N <= 0) return S2ST_ERR_ARG;
  // (logits: the dry workspace, never dereferenced; the collapse allocates nothing)
  return dry_run_floats(e, [&] { return e->forward_speech(nullptr, nullptr, nullptr, B, N, e->ws, 0, nullptr, nullptr); });
}

int s2st_w2v_ctc_forward(s2st_engine* e, const float* wave, const int32_t* sample_lens, const int32_t* frame_lens, int32_t B,
                         int32_t N, int32_t blank, float* logits_out, int32_t* ids_out, int32_t* counts_out,
                         float* workspace, int64_t workspace_floats, void* stream) {
  if (!e || !e->is_speech(s2st_engine::SpeechVariant::LayerNormPreLN) || !e->P || !wave || !sample_lens || !frame_lens ||
      !logits_out || (ids_out && !counts_out))
    return S2ST_ERR_ARG;
  if (B <= 0 || N <= 0) return S2ST_ERR_SHAPE;
  if (!workspace) return S2ST_ERR_WORKSPACE;
  e->begin_call(workspace, workspace_floats, stream);
  if (int rc = e->params_ready()) return rc;  // (frozen weights, as in s2st_hubert_forward)
  return e->end_call(e->forward_speech(wave, sample_lens, frame_lens, B, N, logits_out, blank, ids_out, counts_out));
}

// ---- HiFi-GAN vocoder ---------------------------------------------------------------------------
int s2st_hifigan_create(const s2st_hifigan_config* cfg, s2st_engine** out) {
  if (!cfg || !out || cfg->n_ups < 1 || cfg->n_ups > 8 || cfg->n_kernels < 1 || cfg->n_kernels > 4) return S2ST_ERR_ARG;
  if (cfg->in_dim < 8 || cfg->in_dim % 8) return S2ST_ERR_SHAPE;
  for (int i = 0; i <= cfg->n_ups; ++i) {  // every convolution's input channels: a multiple of 8 (16-byte rows)
    const int ch = cfg->initial_channel >> i;
    if (ch < 8 || ch % 8 || (ch << i) != cfg->initial_channel) return S2ST_ERR_SHAPE;
  }
  for (int i = 0; i < cfg->n_ups; ++i) {
    const int u = cfg->up_rates[i], k = cfg->up_kernels[i];
    if (u < 1 || u > 8 || k < u || (k + u - 1) / u > 64) return S2ST_ERR_SHAPE;
  }
  for (int j = 0; j < cfg->n_kernels; ++j) {
    if (cfg->rb_kernels[j] < 1 || cfg->rb_kernels[j] % 2 == 0) return S2ST_ERR_SHAPE;  // "same" padding needs an odd k
    for (int l = 0; l < 3; ++l)
      if (cfg->rb_dilations[j][l] < 1 || (cfg->rb_kernels[j] - 1) * cfg->rb_dilations[j][l] > 64) return S2ST_ERR_SHAPE;
  }
  s2st_engine* e = new s2st_engine();
  e->kind = s2st_engine::Kind::HifiGan;
  e->gc = *cfg;
  e->c = s2st_model_config{};
  e->c.precise = cfg->precise;
  read_switches(e->sw, e->kind);
  e->build_params_hifigan();
  *out = e;
  return 0;
}

int64_t s2st_hifigan_out_samples(const s2st_engine* e, int32_t T) {
  if (!e || e->kind != s2st_engine::Kind::HifiGan) return S2ST_ERR_ARG;
  return e->hifigan_samples(T);
}

int64_t s2st_hifigan_workspace_floats(s2st_engine* e, int32_t B, int32_t T_max) {
  if (!e || e->kind != s2st_engine::Kind::HifiGan) return S2ST_ERR_ARG;
  return dry_run_floats(e, [&] { return e->forward_hifigan(nullptr, nullptr, B, T_max, nullptr); });
}

int s2st_hifigan_forward(s2st_engine* e, const float* mel, const int32_t* frames, int32_t B, int32_t T, float* wave_out,
                         float* workspace, int64_t workspace_floats, void* stream) {
  if (!e || e->kind != s2st_engine::Kind::HifiGan || !e->P || !mel || !frames || !wave_out) return S2ST_ERR_ARG;
  e->begin_call(workspace, workspace_floats, stream);
  if (int rc = e->params_ready()) return rc;  // (frozen weights, as in s2st_hubert_forward)
  return e->end_call(e->forward_hifigan(mel, frames, B, T, wave_out));
}

}  // extern "C"
