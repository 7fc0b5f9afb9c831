// engine.h -- the engine behind the s2st_engine handle: its state, the types of that state and the declarations of
// every member function.  The definitions live in the units engine_{params,runtime,ops,decode,convnets,speech_encoder,
// hifigan,step}.cpp; engine.cpp holds the extern "C" surface.  Only the small helpers that every op calls many times
// per step are defined here (inline).
//
// s2st training engine: forward + loss + backward of the s2st_transformer as one stream-ordered
// schedule of HIP kernels over flat parameter / gradient arenas and a bump-allocated
// activation workspace.  No tracing compiler, no autograd graph: the forward pushes one
// backward closure per op on a tape; the backward pops them.  Parameters are laid out in
// forward-use order so the backward finishes gradient ranges back-to-front, which lets the
// host overlap RCCL all-reduce of finished ranges with the rest of the backward.
//
// Reference behaviour reproduced (file:line under /root/reference):
//   encoder   examples/s2s_trans/models/s2st_transformer.py:94-140, 195-237
//   decoder   s2st_transformer.py:369-456 ; Prenet/Postnet fairseq/models/text_to_speech/tacotron2.py:85-126
//   layers    fairseq/modules/transformer_layer.py:107-165, 301-446 ; MHA multihead_attention.py:160-385
//   aux text decoders  s2st_transformer.py:483-578 ; transformer_decoder.py:253-378
//   criterion examples/s2s_trans/criterions/s2st_loss.py:179-315
// Layout: activations are [B][T][C] row-major (the reference is [T][B][C]); padded rows are
// computed exactly as the reference computes them.
#ifndef S2ST_ENGINE_H
#define S2ST_ENGINE_H

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

#include "s2st_ops.h"

// The plain types of the engine's state.  A named namespace: s2st_engine is one global type, so every unit must see the
// same member types.
namespace s2st_eng {

struct PInfo {
  std::string name;
  long off, numel;
  int ndim;
  int shape[4];
  int is_buffer;
};

struct Ten {  // plain [rows][cols] fp32 activation
  float* d = nullptr;
  float* g = nullptr;
  // fast (bf16-operand) mode: bf16 copies of d / g with row stride hld(), made by the producer
  // kernel when it can, else by a cast kernel at the first GEMM that reads them
  bf16raw* h = nullptr;
  bf16raw* gh = nullptr;
  int rows = 0, cols = 0;
  bool needs_grad = true;
  bool want_gh = false;  // the gradient is consumed as a GEMM operand: its producer writes gh too
  bool gh_only = false;  // ... and ONLY as that operand (fused attention's O): the producer writes no fp32 gradient (g stays allocated, unwritten)
  // output of conv() whose data gradient reads a bf16 halo image [B][Th][O] (rows at pad + stride * t, zeros elsewhere):
  // the closure that produces this tensor's gradient (BatchNorm / GLU backward) writes the image itself and leaves it in
  // gimg; conv()'s closure then skips its own image pass
  bool img_want = false;
  int img_B = 0, img_Tout = 0, img_Th = 0, img_pad = 0, img_stride = 1;
  bf16raw* gimg = nullptr;
  bool resid_in_loss = false;  // post-net output: the loss root already added this gradient into feat's (post = feat + postnet(feat))
  // produced by linear(act = ReLU, dropout p) with a single consumer (FFN hidden): the consumer's
  // data-gradient GEMM applies the activation backward + bias gradient in its epilogue and leaves the
  // ready bf16 operand in gpre_h (no fp32 gradient of this tensor is ever written)
  int act_mode = 0;
  float act_p = 0.f;
  long act_bias = -1;
  // produced by linear(no activation, dropout p) [+ residual]: the layer norm that consumes it first (hence last
  // in the backward, when its gradient is complete) emits the bf16 operand dropout'(g) + bias gradient (gpre_h)
  bool drop2_ok = false, ln_seen = false;
  float drop2_p = 0.f;
  uint64_t drop2_seed = 0;
  long drop2_bias = -1;
  bool lin_plain = false;  // output of a bias-only linear (no activation / dropout / residual): its gradient IS the GEMM operand
  bf16raw* gpre_h = nullptr;
  long n() const { return (long)rows * cols; }
  int hld() const { return (cols + 7) & ~7; }
};

struct LinP { long w, b; int N, K; };           // offsets into the param arena (b < 0: no bias)
struct LNP { long g, b; int C; };
struct AttnP { long kvq_w, kvq_b, out_w, out_b; };                 // self: [3C][C] k,v,q rows
struct XAttnP { long kv_w, kv_b, q_w, q_b, out_w, out_b; };         // cross: kv [2C][Cenc]
struct EncLayerP { AttnP sa; LNP ln1; LinP fc1, fc2; LNP ln2; };
struct DecLayerP { AttnP sa; LNP ln1; XAttnP xa; LNP ln2; LinP fc1, fc2; LNP ln3; };
struct ConvP { long w, b; int O, I, Kw; };
struct BNP { long g, b, rm, rv; int C; };
struct AuxP {
  long embed; int V, in_dim, d, layers, out_dim;
  long proj_in;  // -1 if none
  std::vector<DecLayerP> L;
  LNP ln; bool has_ln;
  long proj_out; // -1 if none
  long out_proj;
};

}  // namespace s2st_eng

struct s2st_engine {
  using PInfo = s2st_eng::PInfo;
  using Ten = s2st_eng::Ten;
  using LinP = s2st_eng::LinP;
  using LNP = s2st_eng::LNP;
  using AttnP = s2st_eng::AttnP;
  using XAttnP = s2st_eng::XAttnP;
  using EncLayerP = s2st_eng::EncLayerP;
  using DecLayerP = s2st_eng::DecLayerP;
  using ConvP = s2st_eng::ConvP;
  using BNP = s2st_eng::BNP;
  using AuxP = s2st_eng::AuxP;

  // ==== configuration and switches ==============================================================================
  s2st_model_config c;
  // what the handle was created as: the s2st / s2t transformer, or one of the frozen forward-only networks in the same
  // engine object (engine_speech_encoder.cpp, engine_hifigan.cpp)
  enum class Kind { Transformer, SpeechEncoder, HifiGan };
  Kind kind = Kind::Transformer;
  int ffn_act = 1;        // 1 relu (s2st layers), 2 gelu (the speech encoders' layers)
  // the speech encoders (engine_speech_encoder.cpp)
  enum class SpeechVariant { GroupNormPostLN, LayerNormPreLN };
  SpeechVariant sv = SpeechVariant::GroupNormPostLN;
  s2st_w2v_ctc_config sc{};  // (s2st_hubert_config is its prefix: vocab = 0 there)
  bool is_speech(SpeechVariant v) const { return kind == Kind::SpeechEncoder && sv == v; }
  // HiFi-GAN (engine_hifigan.cpp)
  s2st_hifigan_config gc{};

  // Every field that comes from the environment.  Filled once, at create, by read_switches() (engine.cpp): the
  // transformer's create reads the whole table; the speech encoders' create reads the three marked "every kind" plus
  // S2ST_F32_OPERANDS and S2ST_NO_FLASH; the HiFi-GAN create only the three marked "every kind".  What a create path does
  // not read stays at the default written here.  (S2ST_DEC_OVERLAP is not in the table: it is read per call, forward().)
  struct Switches {
    bool overlap_aux = true;  // S2ST_NO_AUX_OVERLAP=1 (A/B switch)
    bool hoist_kv = true;     // S2ST_NO_KV_HOIST=1 (A/B switch): cross-attention K|V projections inside the layers
    bool use_ln_skinny = true; // S2ST_NO_LN_SKINNY=1 (A/B switch): separate layer-norm kernels in the AR decoding steps
    bool use_skinny = true;    // S2ST_NO_SKINNY=1 (A/B switch): tiled GEMMs for the AR decoding steps too
    bool use_ln_fuse = true;  // S2ST_NO_LN_FUSE=1 (A/B switch): separate dropout-backward prologue pass
    bool use_only_h = true;  // S2ST_NO_ONLY_H=1: always keep the fp32 copy of GEMM-only tensors (A/B switch)
    // S2ST_ATTN_GFUSE (default 1): the attention backward emits the bf16 projection gradients itself (no fp32 gradient, no
    // cast pass: ~30 launches fewer on the data path); the modes differ in where the projections' bias gradients come from
    // (attention block, engine_ops.cpp).  1 (default since round 3): out of the kernels' fp32 accumulators BEFORE rounding, as
    // per-(block, wave) partial sums by DPP row reductions, folded in a fixed order with the segment's layer-norm partials --
    // exact (a key bias's mathematically zero gradient stays ~0) and run-to-run identical; 2: the same sums as fp32 atomics; 3:
    // column sums of the ROUNDED copies (round 1's form: a rounding residue instead of ~0 that changes with any upstream ulp --
    // multi-update trajectories of cold processes then repeat in ~85 % of runs); 0: off (fp32 gradients +
    // cast pass).
    bool use_attn_gfuse = true;
    int attn_gfuse_mode = 1;
    // Ordered sums (default since round 3; S2ST_ORDERED_BIAS_SUMS=0 restores the atomics, an A/B switch): every sum that
    // used fp32 atomics -- bias-gradient column sums (linear backward prologue, conv biases, the masked data-gradient
    // GEMM epilogue), embedding-row gradients, the decoder's position scale -- is formed as partial rows + a fold in index
    // order, so a gradient is a function of (parameters, batch, seed) down to the last bit.  Round 2 had this as an
    // option at +3 % of a step (one small fold launch per sum); the folds now ride in the segment's batched fold launch
    // (pending_lnfold), i.e. cost no launches of their own.
    bool ordered_sums = true;
    bool use_act_fuse = true;  // S2ST_NO_ACT_FUSE=1: separate ReLU-dropout backward kernel (A/B switch)
    bool use_flash = true;  // S2ST_NO_FLASH=1: unfused attention everywhere (A/B switch)
    // S2ST_ATTN_KEEP_F32=1 (A/B switch; every kind): the fused attention also stores O in fp32 and the out-projection's
    // data-gradient GEMM also stores dO in fp32, although every reader takes the bf16 copies
    bool attn_keep_f32 = false;
    // S2ST_CONVNET_FUSE=0 (A/B switch; every kind): BatchNorm statistics finalize / backward fold / the convolutions' gradient
    // halo images / the post-net residual add as launches of their own
    bool convnet_fuse = true;
    bool f32_operands = false;  // debug A/B switch S2ST_F32_OPERANDS=1: bf16 MFMA on fp32-stored operands
    // weight-gradient GEMMs waiting for their group launch (S2ST_NO_WGRAD_GROUP=1: A/B switch, one launch each)
    bool group_wgrad = true;
    int group_flush_at = 6;  // S2ST_WGRAD_GROUP=<n>: problems per launch (<= S2ST_GROUP_MAX); measured 2 .. 8 on the bench
                             // workload: 12.25 / 10.99 / 10.56 / 10.44 / 10.46 ms per step for 2 / 3 / 4 / 6 / 8
    bool ln_bwd_split = false;  // S2ST_LN_BWD_SPLIT=1 (A/B switch): round 2's separate parameter-gradient pass
    // S2ST_STALL_TRACE=1: time spent by the data-path stream in each cross-stream wait (timing events around the
    // wait; read back by s2st_engine_stall_report after the caller synchronised)
    bool stall_trace = false;
    // S2ST_GEMM_STREAMK=1 (every kind): bind stream-K scratch buffers to the two streams (opt-in: on the products of this step
    // the hand-off costs more than the idle tail it removes -- gemm_bf16.hip streamk_mode())
    bool use_streamk = false;
    bool side_stream = true;  // S2ST_NO_SIDE_STREAM=1: the switch half of side_allowed
  } sw;
  bool fast() const { return c.precise == 0 && !sw.f32_operands; }

  // ==== arenas ==================================================================================================
  std::vector<PInfo> infos;
  long n_params = 0, n_buffers = 0;
  float *P = nullptr, *G = nullptr, *BUF = nullptr;
  bf16raw* PH = nullptr;  // bf16 copy of the parameter arena (same offsets), refreshed every forward
  bool ph_fresh = false;   // s2st_engine_bf16_is_fresh: PH already equals bf16(P) for the next forward
  bf16raw* PHT = nullptr;  // optional: transposed bf16 copies of the 2-D weights (same offsets): the
                           // data-gradient GEMMs then read K-contiguous operands (~25 % faster here)
  bool pht_valid = false;
  struct WT { long off; int N, K; };
  std::vector<WT> wt_list;  // the [N][K] matrices linear() multiplies by (fused k|v|q blocks as ONE matrix)
  void reg_wt(long off, int N, int K) { if (N % 8 == 0 && K % 8 == 0) wt_list.push_back(WT{off, N, K}); }
  bool has_wt(long off, int N, int K) const {
    if (!pht_valid) return false;
    for (const WT& t : wt_list) if (t.off == off && t.N == N && t.K == K) return true;
    return false;
  }
  std::vector<s2st_transpose_table> wt_tables;

  // ==== the second stream, its events and the schedule's tape indices ==========================================
  // weight-gradient GEMMs are off the backward critical path: they run on a second stream, next
  // to the data-gradient chain (each of these GEMMs alone fills about half of the 256 CUs)
  hipStream_t side_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_taps_ = nullptr;
  hipEvent_t ev_kv_ = nullptr;
  bool kv_wait_ = false;    // the data path has not yet waited for the hoisted K|V projections
  hipEvent_t ev_auxb_ = nullptr;
  size_t aux_wait_idx = 0, aux_lo_idx = 0, aux_hi_idx = 0;  // tape indices: tap-LN end; aux section [lo, hi)
  bool aux_bwd_on_side = false;
  // S2ST_DEC_OVERLAP=<bit mask> (per call, default 3; 0 = everything below in tape order on the data path): mel-decoder work
  // that does not depend on the encoder, or that the encoder's backward does not depend on, runs on the second stream
  //   bit 0  forward: prenet, positions, layer 0's self-attention block and cross-attention query projection read only
  //          prev_output_tokens -- issued on the second stream ahead of the encoder (forward(): dec_early)
  //   bit 1  backward: everything of layer 0 below its cross-attention's dK|dV (query projection ... prenet) produces
  //          parameter gradients only -- tape range [tail_lo_idx, tail_hi_idx) on the second stream
  // (A third piece was built and measured: each hoisted K|V projection's backward on the second stream right behind its
  //  layer's cross-attention.  The data path then has to wait for the encoder output's gradient behind the second stream's
  //  backlog of weight-gradient products, ~0.75 ms at that point of the step: +0.26 ms per step, left out --
  //  profiles/r07_dec_overlap_pieces_ab.txt.)
  int dec_overlap = 3;
  hipEvent_t ev_head_ = nullptr;    // the block issued ahead (bit 0) is complete
  // every event of the second stream was created (by the calls' results, not by the handles: the CPU emulator's events are
  // null handles, and S2ST_DEC_OVERLAP has to engage there for tests/test_decoder_overlap.py to check its re-ordering)
  bool side_events_ = false;
  size_t tail_lo_idx = 0, tail_hi_idx = 0;
  bool tail_bwd_on_side = false, tail_side_ = false;  // tail_side_: st_ points at the second stream for the tail's closures
  bool dec_early_active = false;    // the last forward issued the block ahead, on the second stream (s2st_engine_dec_overlap_active)
  size_t xattn0_idx = 0;            // tape index of the closure of mel-decoder layer 0's cross-attention (0: none)
  bool side_used = false;
  float* skws_side = nullptr;
  bool side_allowed = false;  // bf16-operand mode and no S2ST_NO_SIDE_STREAM=1
  bool side_tried = false;
  struct Stall { const char* what; hipEvent_t a, b; };
  std::vector<Stall> stalls;  // sw.stall_trace

  // ==== per-call state ==========================================================================================
  float* ws = nullptr;
  long ws_cap = 0, ws_top = 0, ws_peak = 0;
  bool dry = false, oom = false;
  int err = 0;
  hipStream_t st_ = nullptr;
  std::vector<std::function<void()>> tape;
  std::vector<Ten*> tens;
  struct Mark { size_t tape_idx; long param_off; };
  std::vector<Mark> marks;
  long param_watermark = 0;
  int next_segment = 0;
  uint64_t seed = 0, site = 0;
  float gscale = 1.f;
  s2st_batch bt;
  s2st_outputs outs;
  float* skws = nullptr;  // split-K partial-sum scratch of the weight-gradient GEMMs (per call)
  long skws_n = 0;
  bool stop_after_encoder = false;
  Ten* enc_out_keep = nullptr;
  const int* gan_frames = nullptr;

  // ==== parameter handles: the transformer =====================================================================
  ConvP sub[2];
  std::vector<EncLayerP> enc;
  LNP enc_ln; bool has_enc_ln = false;
  LNP asr_norm, st_norm;
  long pos_alpha = 0;
  std::vector<LinP> prenet;   // prenet_layers + 1
  std::vector<DecLayerP> dec;
  LNP dec_ln; bool has_dec_ln = false;
  LinP feat_proj, eos_proj;
  std::vector<ConvP> post_conv;
  std::vector<BNP> post_bn;
  LinP ctc_proj, ctc_proj_tgt;
  AuxP asr, st;
  AuxP s2t;  // s2t_mode: the model's own text decoder ("decoder.*")
  long enc_spk = -1, dec_spk = -1;  // speaker-embedding tables (n_speakers > 0)
  LinP enc_spk_proj{-1, -1, 0, 0};  // t2s text encoder: spk_emb_proj over cat[x, emb] (t2s_transformer.py:43-46, 107-111)
  // t2s text encoder front
  long enc_embed = -1, enc_pos_alpha = -1;
  std::vector<ConvP> enc_conv;
  std::vector<BNP> enc_bn;
  LinP enc_prenet_proj;

  // ==== parameter handles: the speech encoders ==================================================================
  struct SpeechP {
    long conv_w[8], conv_b[8]; LNP conv_ln[8];  // GroupNormPostLN: no biases, and only conv_ln[0] (the GroupNorm's affine)
    LNP ln; LinP proj; long pos_w, pos_b; std::vector<EncLayerP> L; LNP enc_ln;
    LinP lm;  // LayerNormPreLN only
  } sp;
  // the variants' state_dict names: checkpoints and the host wrappers' tables depend on names, order and shapes
  struct SpeechNames {
    const char *conv, *conv_w, *conv_norm, *ln, *proj, *pos, *layers, *attn, *ln1, *fc1, *fc2, *enc_ln;
  };

  // ==== parameter handles: HiFi-GAN =============================================================================
  struct GanConv { long w, b; int cin, cout, k, dil; };
  struct GanP { GanConv pre, post; GanConv ups[8]; std::vector<GanConv> c1, c2; } gp;  // c1 / c2: [stage][rb][layer]

  // ==== decode state =============================================================================================
  // ---- AR decoding state (config 5): caller-owned cache buffer laid out by decode_begin --------
  // replay_ != null: decode_step in its graph-replayable form (s2st_engine_decode_step_replay): the step, the prenet's dropout
  // seeds, the input frame, the position row and the output rows are read from / written to the fixed device buffers of *replay_
  const s2st_decode_replay* replay_ = nullptr;
  // merged decode batches (s2st_engine_decode_row_map): device [B] -- the row of its OWN batch whose Prenet dropout mask row b draws
  const int* dec_row_map = nullptr;
  struct Dec {
    float* base = nullptr; int B = 0, E = 0, maxT = 0; const int* enc_lens = nullptr; const float* pe_dec = nullptr;
    float* pe_alpha = nullptr;  // [maxT + 2][dec_dim]: pos_emb_alpha * PE rows (tail of the caller's state buffer)
  } dec_st;
  float* dec_selfK(int l) const { return dec_st.base + (long)l * 2 * dec_st.B * dec_st.maxT * c.dec_dim; }
  float* dec_selfV(int l) const { return dec_selfK(l) + (long)dec_st.B * dec_st.maxT * c.dec_dim; }
  float* dec_crossKV(int l) const {
    return dec_st.base + (long)c.dec_layers * 2 * dec_st.B * dec_st.maxT * c.dec_dim + (long)l * dec_st.B * dec_st.E * 2 * c.dec_dim;
  }
  // incremental decoding of an aux ASR / ST text decoder (engine_decode.cpp): the caller-owned state buffer
  struct AuxInc {
    float* base = nullptr; int Bb = 0, E = 0, maxT = 0, cur = 0; const int* enc_lens = nullptr;
  } aux_inc[2];
  static long aux_inc_half(const AuxP& a, int Bb, int maxT) { return (long)a.layers * 2 * Bb * maxT * a.d; }
  float* aux_selfK(const AuxP& a, const AuxInc& S, int l, int buf) const {
    return S.base + (long)buf * aux_inc_half(a, S.Bb, S.maxT) + (long)l * 2 * S.Bb * S.maxT * a.d;
  }
  float* aux_crossKV(const AuxP& a, const AuxInc& S, int l) const {
    return S.base + 2 * aux_inc_half(a, S.Bb, S.maxT) + (long)l * S.Bb * S.E * 2 * a.d;
  }

  // ==== the overlapped optimizer's chunk events (engine_runtime.cpp) ============================================
  std::vector<hipEvent_t> adam_ev;
  std::vector<long> adam_lo;      // first element of chunk i
  int adam_next = 0;              // chunks [0, adam_next) have been waited for by the data-path stream
  bool adam_pending = false;

  // ==== the pending weight-gradient and fold queues (engine_runtime.cpp) ========================================
  std::vector<GemmArgs> pending_wgrad;  // sw.group_wgrad, sw.group_flush_at
  // layer-norm parameter gradients: the backward row kernels leave column-sum partials; one batched fold per backward
  // segment (or per S2ST_LNFOLD_MAX layer norms) adds them to the gradient arena.  Parameter gradients only: the fold
  // runs on the second stream behind everything enqueued on the stream the row kernels ran on.
  s2st_lnfold_table pending_lnfold{};

  // ==== the dropout-site log ====================================================================================
  // Dropout sites: the seed of the n-th site of a forward is a function of (batch seed, n).  s2st_engine_site_log(e, 1)
  // makes the forward also RECORD every site -- seed, kind, p, the element geometry its mask is indexed by and where in
  // the model it sits -- so that a test can regenerate the keep masks (s2st_dropout_f32 over ones) and hand them to the CPU
  // oracle: parity with the recipe's dropouts ON (tests/test_dropout_parity.py).  Nothing on the data path reads the log.
  bool site_log_on = false;
  std::vector<s2st_dropout_site> site_log;
  char site_ctx[24] = "";
  void set_ctx(const char* fmt, int i = 0) { snprintf(site_ctx, sizeof site_ctx, fmt, i); }

  // ==== inline helpers: what every op calls many times per step =================================================
  // arena
  float* alloc(long n, bool zero = false) {
    n = (n + 63) / 64 * 64;
    float* p = nullptr;
    if (ws_top + n > ws_cap) {
      if (!dry) { oom = true; err = S2ST_ERR_WORKSPACE; }
    } else {
      p = ws + ws_top;
    }
    ws_top += n;
    if (ws_top > ws_peak) ws_peak = ws_top;
    if (p && zero && !dry) hipMemsetAsync(p, 0, sizeof(float) * n, st_);
    return p;
  }
  Ten* newT(int rows, int cols, float* ext = nullptr, bool f32 = true) {
    Ten* t = new Ten();
    t->rows = rows; t->cols = cols;
    t->d = ext ? ext : (f32 ? alloc(t->n()) : nullptr);
    tens.push_back(t);
    return t;
  }
  // gradient buffer of t: first request allocates it (acc = false: caller must overwrite),
  // later requests accumulate
  float* gradbuf(Ten* t, bool& acc) {
    if (t->g) { acc = true; return t->g; }
    t->g = alloc(t->n());
    acc = false;
    return t->g;
  }
  bf16raw* alloc_h(long n) { return reinterpret_cast<bf16raw*>(alloc((n + 1) / 2)); }
  bool live() const { return !dry && !oom && err == 0; }
  void chk(int rc) { if (rc && !err) err = rc; }
  float* ws_for(hipStream_t s) const { return (side_ && s == side_) ? skws_side : skws; }
  void mark() { marks.push_back(Mark{tape.size(), param_watermark}); }
  void touch(long off_end) {
    if (off_end > param_watermark) param_watermark = off_end;
    if (adam_pending && st_ != side_) adam_wait_upto(off_end);
  }
  // frozen tables (Embedding.from_pretrained(freeze=True), tasks/s2s_translation.py:161-171) live in the BUFFER arena like
  // the BatchNorm statistics: the reference leaves them out of the optimizer, so neither Adam's sweep over the
  // parameter arena nor weight decay may touch them
  const float* spk_tab(long off) const { return (c.spk_frozen ? BUF : P) + off; }
  void touch_spk(long off_end) { if (!c.spk_frozen) touch(off_end); }
  int n_segments() const { return marks.empty() ? 0 : (int)marks.size() - 1; }

  // ==== engine_params.cpp: parameter construction ===============================================================
  long add(const std::string& name, std::vector<int> shape, int is_buffer = 0);
  LinP add_lin(const std::string& pre, int N, int K, bool bias = true);
  LNP add_ln(const std::string& pre, int C);
  AttnP add_self_attn(const std::string& pre, int C);
  XAttnP add_cross_attn(const std::string& pre, int C, int Cenc);
  DecLayerP add_dec_layer(const std::string& pre, int C, int ffn, int Cenc);
  AuxP add_aux(const std::string& pre, int V, int in_dim, int d, int layers, int out_dim = 512);
  void build_params();

  // ==== engine_runtime.cpp: second stream, casts, seeds, the overlapped Adam, the queues ========================
  void ensure_side();
  hipStream_t fork_side();
  void join_side();
  void wait_traced(hipStream_t st, hipEvent_t ev, const char* what);
  bf16raw* half_of(Ten* t);
  bf16raw* ghalf_of(Ten* t);
  bf16raw* cast_buf(const float* x, long n);
  bf16raw* cast_halo(const float* img, int B, int T, int pad, int C, bool plain = false);
  uint64_t next_seed(int kind, float p, long d0, long d1 = 0, long d2 = 0, long d3 = 0, long d4 = 0);
  void adam_wait_upto(long off_end);
  int adam_overlapped(float* m, float* v, const float* sumsq, int nparts, float gmul, const float* gmul_dev, float max_norm,
                      float lr, float b1, float b2, float eps, float wd, int step, float* gnorm_out, int* skipped, int use_ph,
                      int nchunks, hipStream_t main);
  void adam_wait_all(hipStream_t stream);
  void push_wgrad(const GemmArgs& g);
  void flush_wgrad();
  void flush_lnfold();
  void add_fold(const float* part, int nblocks, int cols, float* out);
  void build_wt_tables();

  // ==== engine_ops.cpp: the ops of the training graph ===========================================================
  Ten* linear(Ten* x, long w, long b, int N, int K, int act = 0, float drop_p = 0.f,
              Ten* resid = nullptr, float* ext_out = nullptr, bool only_h = false, const float* resid_row = nullptr);
  Ten* ln_linear(Ten* x, const LNP& ln, long w, long b, int N, int K, int act = 0, float* ext_out = nullptr);
  Ten* layernorm(Ten* x, const LNP& p, float* ext_out = nullptr, bool only_h = false);
  // attention core.  q: [B*T] rows at qp (+ h*dh), ld ldq ; k/v rows [B*S] ; out [B*T][C]
  struct AttnIO {
    Ten* qt; int qoff, ldq;     // tensor holding q, column offset, row stride
    Ten* kt; int koff, ldk;
    Ten* vt; int voff, ldv;
  };
  Ten* attention(const AttnIO& io, int B, int T, int S, int H, int dh, const int* klen, int causal,
                 float drop_p, float* attn_mean_out /* [B][S][T] or null */, const float* guided_sum = nullptr);
  Ten* self_attn_block(Ten* x, const AttnP& a, int B, int T, int H, const int* klen, int causal,
                       Ten* resid);
  Ten* cross_kv(Ten* encx, const XAttnP& a, int C);
  Ten* cross_attn_block(Ten* q, Ten* encx, const XAttnP& a, int B, int T, int S, int H,
                        const int* klen, Ten* resid, float* attn_mean_out, Ten* kv_pre = nullptr,
                        const float* guided_sum = nullptr);
  Ten* ffn_block(Ten* x, const LinP& fc1, const LinP& fc2, Ten* resid);
  Ten* enc_layer(Ten* x, const EncLayerP& l, int B, int T);
  // The part of a decoder layer that does not read the encoder: the self-attention block and the cross-attention's query
  // projection.  x: the residual stream behind the self-attention block; q: the projected queries.
  struct DecHead { Ten* x = nullptr; Ten* q = nullptr; };
  DecHead dec_head(Ten* x, const DecLayerP& l, int B, int T, int H, bool pre_ln, const int* self_klen);
  Ten* dec_layer(Ten* x, Ten* encx, const DecLayerP& l, int B, int T, int S, int H, bool pre_ln,
                 const int* self_klen, float* attn_mean_out, Ten* kv_pre = nullptr, const DecHead* head = nullptr,
                 const float* guided_sum = nullptr);
  struct ConvIn { float* xh; Ten* src; int Tin; const bf16raw* xhh; };  // src: plain tensor whose grad we produce (or null); xhh: bf16 twin of xh
  struct ConvW { float *wf, *wd, *dwf; const bf16raw *wfh, *wdh; };
  Ten* conv(const ConvIn& in, const ConvP& p, int B, int stride, const ConvW& cw);
  Ten* glu_to(Ten* z, float* y, Split ysp, int Cc, bf16raw* imgh = nullptr, int B = 0, int T = 0, int pad = 0);
  Ten* add_pe(Ten* x, const int* pos, const float* table, float scale, long alpha_off, float drop_p, long spk_off = -1,
              int T = 0);
  Ten* aux_decoder(const AuxP& a, Ten* tap, const long* prev_tok, const int* pos, const int* lens, int B,
                   int L, const float* pe, float* logits_out);

  // ==== engine_decode.cpp: incremental decoding =================================================================
  Ten* dec_attn(Ten* qt, int qoff, float* K, float* V, long ldk, long kbs, const int* klen, int nkeys,
                int H, float* attn_mean, int S, const float* k_new = nullptr, const float* v_new = nullptr, long ld_new = 0,
                int pos_new = 0, int kv_bf16 = 0, const int* step_ptr = nullptr, int dim = 0, int rows = 0);
  int aux_inc_begin(const AuxP& a, AuxInc& S, Ten* tap);
  int aux_inc_step(const AuxP& a, AuxInc& S, int step, const long* tokens, const int* reorder, const int* pos, const float* pe,
                   float* logits_out);
  int decode_step(int step, const float* prev, const int* pos, const int* self_klen, uint64_t sd, float* feat_out,
                  float* eos_prob, float* attn_out);

  // ==== engine_convnets.cpp: the convolutional sub-networks =====================================================
  ConvW make_conv_scratch(const ConvP& p, bool need_wd, bool tr);
  bool bn_bwd_fusable(const Ten* z, int C) const;
  bf16raw* bn_bwd_image(Ten* z, int B, int T);
  Ten* postnet(Ten* feat, int B, int D, bool tr, std::vector<ConvW>& csp, float* post_out);
  Ten* text_prenet(Ten* emb, int B, int T, bool tr, std::vector<ConvW>& csp);

  // ==== engine_speech_encoder.cpp: the two frozen speech encoders ===============================================
  static const SpeechNames& speech_names(SpeechVariant v);
  void build_params_speech();
  int speech_frames(int n) const;
  int forward_speech(const float* wave, const int* sample_lens, const int* frame_lens, int B, int N, float* out, int blank,
                     int* ids_out, int* counts_out);

  // ==== engine_hifigan.cpp: the HiFi-GAN generator ==============================================================
  GanConv add_gan_conv(const std::string& pre, int cin, int cout, int k, int dil, int phases = 1);
  void build_params_hifigan();
  int gan_extra(int i) const;
  long hifigan_samples(int T) const;
  void gan_conv(const GanConv& cv, const void* in, bool in_f32, int lin, int lout, int nq, int up, const int* off,
                int la_in, int lb_in, int la_out, int lb_out, const float* resid, float* out, void* img, float slope,
                int mrf = 0);
  int forward_hifigan(const float* mel, const int* frames, int B, int T, float* wave);

  // ==== engine_step.cpp: one step ===============================================================================
  void reset_call();
  void begin_call(float* workspace, long workspace_floats, void* stream);
  int params_ready(bool chunked = false, bool refresh = true);
  int end_call(int rc);
  int forward();
  int forward_s2t(Ten* enc_out, bool with_loss);
  int backward_segment(int seg);
};

#endif  // S2ST_ENGINE_H
