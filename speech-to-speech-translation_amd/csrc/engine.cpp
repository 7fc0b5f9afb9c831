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
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "s2st_ops.h"
#include <hip/hip_ext.h>

namespace {

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

}  // namespace

struct s2st_engine {
  s2st_model_config c;
  std::vector<PInfo> infos;
  long n_params = 0, n_buffers = 0;
  float *P = nullptr, *G = nullptr, *BUF = nullptr;
  // weight-gradient GEMMs are off the backward critical path: they run on a second stream, next
  // to the data-gradient chain (each of these GEMMs alone fills about half of the 256 CUs)
  hipStream_t side_ = nullptr;
  hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr, ev_taps_ = nullptr;
  bool overlap_aux = true;  // S2ST_NO_AUX_OVERLAP=1 (A/B switch)
  bool hoist_kv = true;     // S2ST_NO_KV_HOIST=1 (A/B switch): cross-attention K|V projections inside the layers
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
  void ensure_side() {        // the second stream and its events, on first need (the first training forward; the overlapped update)
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
  hipStream_t fork_side() {  // everything issued on st_ so far happens-before what follows on the returned stream
    if (!side_) return st_;
    hipEventRecord(ev_fork_, st_);
    hipStreamWaitEvent(side_, ev_fork_, 0);
    side_used = true;
    return side_;
  }
  // S2ST_STALL_TRACE=1: time spent by the data-path stream in each cross-stream wait (timing events around the
  // wait; read back by s2st_engine_stall_report after the caller synchronised)
  struct Stall { const char* what; hipEvent_t a, b; };
  std::vector<Stall> stalls;
  bool stall_trace = false;
  void wait_traced(hipStream_t st, hipEvent_t ev, const char* what) {
    if (!stall_trace) { hipStreamWaitEvent(st, ev, 0); return; }
    Stall s{what, nullptr, nullptr};
    hipEventCreate(&s.a);
    hipEventCreate(&s.b);
    hipEventRecord(s.a, st);
    hipStreamWaitEvent(st, ev, 0);
    hipEventRecord(s.b, st);
    stalls.push_back(s);
  }
  void join_side() {
    if (!side_ || !side_used) return;
    hipEventRecord(ev_join_, side_);
    wait_traced(st_, ev_join_, "join_side");
    side_used = false;
  }

  // ---- AR decoding state (config 5): caller-owned cache buffer laid out by decode_begin --------
  // replay_ != null: decode_step in its graph-replayable form (s2st_engine_decode_step_replay): the step, the prenet's dropout
  // seeds, the input frame, the position row and the output rows are read from / written to the fixed device buffers of *replay_
  const s2st_decode_replay* replay_ = nullptr;
  // merged decode batches (s2st_engine_decode_row_map): device [B] -- the row of its OWN batch whose Prenet dropout mask row b draws
  const int* dec_row_map = nullptr;
  bool stop_after_encoder = false;
  Ten* enc_out_keep = nullptr;
  struct Dec {
    float* base = nullptr; int B = 0, E = 0, maxT = 0; const int* enc_lens = nullptr; const float* pe_dec = nullptr;
    float* pe_alpha = nullptr;  // [maxT + 2][dec_dim]: pos_emb_alpha * PE rows (tail of the caller's state buffer)
  } dec_st;
  float* dec_selfK(int l) const { return dec_st.base + (long)l * 2 * dec_st.B * dec_st.maxT * c.dec_dim; }
  float* dec_selfV(int l) const { return dec_selfK(l) + (long)dec_st.B * dec_st.maxT * c.dec_dim; }
  float* dec_crossKV(int l) const {
    return dec_st.base + (long)c.dec_layers * 2 * dec_st.B * dec_st.maxT * c.dec_dim + (long)l * dec_st.B * dec_st.E * 2 * c.dec_dim;
  }
  bool use_ln_skinny = true; // S2ST_NO_LN_SKINNY=1 (A/B switch): separate layer-norm kernels in the AR decoding steps
  bool use_skinny = true;    // S2ST_NO_SKINNY=1 (A/B switch): tiled GEMMs for the AR decoding steps too
  bool use_ln_fuse = true;  // S2ST_NO_LN_FUSE=1 (A/B switch): separate dropout-backward prologue pass
  bool use_only_h = true;  // S2ST_NO_ONLY_H=1: always keep the fp32 copy of GEMM-only tensors (A/B switch)
  // S2ST_ATTN_GFUSE (default 1): the attention backward emits the bf16 projection gradients itself (no fp32 gradient, no
  // cast pass: ~30 launches fewer on the data path); the modes differ in where the projections' bias gradients come from
  // (attention block below).  1 (default since round 3): out of the kernels' fp32 accumulators BEFORE rounding, as per-(block,
  // wave) partial sums by DPP row reductions, folded in a fixed order with the segment's layer-norm partials -- exact (a key
  // bias's mathematically zero gradient stays ~0) and run-to-run identical; 2: the same sums as fp32 atomics; 3: column sums of
  // the ROUNDED copies (round 1's form: a rounding residue instead of ~0 that changes with any upstream ulp -- multi-update
  // trajectories of cold processes then repeat in ~85 % of runs); 0: off (fp32 gradients + cast pass).
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
  // S2ST_ATTN_KEEP_F32=1 (A/B switch): the fused attention also stores O in fp32 and the out-projection's data-gradient
  // GEMM also stores dO in fp32, although every reader takes the bf16 copies
  bool attn_keep_f32 = s2st_env_on("S2ST_ATTN_KEEP_F32");
  // S2ST_CONVNET_FUSE=0 (A/B switch): BatchNorm statistics finalize / backward fold / the convolutions' gradient halo
  // images / the post-net residual add as launches of their own
  bool convnet_fuse = s2st_env_int("S2ST_CONVNET_FUSE", 1) != 0;
  int ffn_act = 1;        // 1 relu (s2st layers), 2 gelu (the speech encoders' layers)
  // what the handle was created as: the s2st / s2t transformer, or one of the frozen forward-only networks in the same
  // engine object (engine_speech_encoder.h, engine_hifigan.h)
  enum class Kind { Transformer, SpeechEncoder, HifiGan };
  Kind kind = Kind::Transformer;
  float* ws_for(hipStream_t s) const { return (side_ && s == side_) ? skws_side : skws; }
  float* skws = nullptr;  // split-K partial-sum scratch of the weight-gradient GEMMs (per call)
  long skws_n = 0;
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
  void build_wt_tables() {
    s2st_transpose_table cur{};
    for (const WT& t : wt_list) {
      if (cur.n == S2ST_TRANSPOSE_MAX) { wt_tables.push_back(cur); cur = s2st_transpose_table{}; }
      const int i = cur.n++;
      cur.off[i] = (unsigned)t.off; cur.rows8[i] = (unsigned short)(t.N / 8); cur.cols8[i] = (unsigned short)(t.K / 8);
      cur.tile0[i + 1] = cur.tile0[i] + (unsigned)(((t.N + 63) / 64) * ((t.K + 63) / 64));
    }
    if (cur.n) wt_tables.push_back(cur);
  }
  bf16raw* PH = nullptr;  // bf16 copy of the parameter arena (same offsets), refreshed every forward
  bool f32_operands = false;  // debug A/B switch S2ST_F32_OPERANDS=1: bf16 MFMA on fp32-stored operands
  bool fast() const { return c.precise == 0 && !f32_operands; }

  // parameter handles
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

  // per-call state
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

#include "engine_params.h"  // parameter construction

#include "engine_runtime.h"  // per-call runtime

#include "engine_ops.h"  // the ops of the training graph

#include "engine_decode.h"  // incremental decoding

#include "engine_convnets.h"  // the convolutional sub-networks

#include "engine_speech_encoder.h"  // the frozen HuBERT front end (config 4) and the wav2vec 2.0 CTC recogniser (ASR-BLEU)

#include "engine_hifigan.h"  // the HiFi-GAN vocoder (--vocoder hifigan)

#include "engine_step.h"  // one step

};

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

// The two speech encoders' one create (engine_speech_encoder.h): cfg.vocab is read by the LayerNormPreLN variant only.
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
  // the recogniser: every product goes through the tiled GEMM whatever the batch's row count: an utterance's logits do not
  // depend on what else is in the batch
  if (pre_ln) e->use_skinny = false;
  e->f32_operands = s2st_env_on("S2ST_F32_OPERANDS");
  e->use_flash = !(s2st_env_on("S2ST_NO_FLASH"));
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
  e->f32_operands = s2st_env_on("S2ST_F32_OPERANDS");
  e->use_flash = !(s2st_env_on("S2ST_NO_FLASH"));
  e->group_wgrad = !(s2st_env_on("S2ST_NO_WGRAD_GROUP"));
  if (s2st_env_str("S2ST_WGRAD_GROUP")) {
    e->group_flush_at = atoi(s2st_env_str("S2ST_WGRAD_GROUP"));
    if (e->group_flush_at < 1) e->group_flush_at = 1;
    if (e->group_flush_at > S2ST_GROUP_MAX) e->group_flush_at = S2ST_GROUP_MAX;
  }
  e->use_act_fuse = !(s2st_env_on("S2ST_NO_ACT_FUSE"));
  e->use_only_h = !(s2st_env_on("S2ST_NO_ONLY_H"));
  e->hoist_kv = !(s2st_env_on("S2ST_NO_KV_HOIST"));
  e->stall_trace = s2st_env_on("S2ST_STALL_TRACE");
  e->use_ln_skinny = !(s2st_env_on("S2ST_NO_LN_SKINNY"));
  e->use_skinny = !(s2st_env_on("S2ST_NO_SKINNY"));
  e->use_ln_fuse = !(s2st_env_on("S2ST_NO_LN_FUSE"));
  e->attn_gfuse_mode = s2st_env_int("S2ST_ATTN_GFUSE", 1);
  e->use_attn_gfuse = e->attn_gfuse_mode != 0;
  e->ln_bwd_split = s2st_env_on("S2ST_LN_BWD_SPLIT");
  e->ordered_sums = !(s2st_env_int("S2ST_ORDERED_BIAS_SUMS", 1) == 0);
  e->build_params();
  // (a process that replays HIP graphs can carry a stale "last error" of the runtime's own capture-time queries: the preload's
  //  launch checks must see their own errors only)
  (void)hipGetLastError();
  if (!cfg->precise && (s2st_gemm_bf16_preload(nullptr) != 0 || s2st_flash_attn_preload(nullptr) != 0)) { delete e; return S2ST_ERR_LAUNCH; }
  // The second stream is made at the first TRAINING forward (ensure_side), not here: a process has four hardware queues
  // (runtime/streams.py) and an engine that only ever decodes would hold one of them for nothing -- the caller's stream
  // then shares a queue with one of the generator's chains (config 5, profiles/r05_queue_matrix.txt).
  e->side_allowed = !cfg->precise && !(s2st_env_on("S2ST_NO_SIDE_STREAM"));
  e->overlap_aux = !(s2st_env_on("S2ST_NO_AUX_OVERLAP"));
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
  if (!e || !e->dec_st.base || !e->dec_st.pe_alpha || !e->fast() || !e->PH || !e->use_skinny) return 0;
  const int B = e->dec_st.B, Cd = e->c.dec_dim;
  if (B < 1 || B > 64 || e->c.prenet_dim % 32 || e->c.out_dim % 32 || Cd % 64 || e->c.prenet_layers > 7) return 0;
  if (e->has_dec_ln && !e->use_ln_skinny) return 0;
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
