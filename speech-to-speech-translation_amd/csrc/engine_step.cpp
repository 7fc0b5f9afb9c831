// engine_step.cpp -- one step: the forward schedule (encoder, decoder, post-net, aux heads, losses) and the backward over
// tape segments.
#include <cmath>
#include <iterator>

#include "engine.h"

using namespace s2st_eng;

// ------------------------------------------------------------------------------------
void s2st_engine::reset_call() {
  pending_wgrad.clear();
  pending_lnfold = s2st_lnfold_table{};
  s2st_gemm_streamk_unbind_all();  // the scratch lives in the previous call's workspace
  for (Ten* t : tens) delete t;
  tens.clear();
  tape.clear();
  marks.clear();
  ws_top = 0;
  ws_peak = 0;
  oom = false;
  err = 0;
  site = 0;
  site_log.clear();
  xattn0_idx = 0;
  tail_bwd_on_side = tail_side_ = dec_early_active = false;
  site_ctx[0] = 0;
  param_watermark = 0;
  next_segment = 0;
  skws = nullptr; skws_n = 0; skws_side = nullptr;  // (forward() allots them; the backward segments reuse them)
}
// prologue of every call that launches work: a fresh call on `stream` with the caller's workspace
void s2st_engine::begin_call(float* workspace, long workspace_floats, void* stream) {
  reset_call();
  dry = false;
  ws = workspace;
  ws_cap = workspace_floats;
  st_ = (hipStream_t)stream;
}
// The one place that decides whether this call may read the parameters: P once a pending overlapped update has landed
// on st_; in fast mode PH too, cast from P here unless the caller vouched for it (s2st_engine_bf16_is_fresh).
// chunked: the caller waits for the update chunk by chunk as it reads (touch(): forward), so the whole-arena wait is
//   needed only before the cast -- when the update itself wrote PH, it is skipped.
// refresh = false: a step of a run whose begin call made PH (decode / incremental aux steps): no cast, ph_fresh kept.
int s2st_engine::params_ready(bool chunked, bool refresh) {
  if (dry) return 0;
  const bool fm = fast();
  if (fm && !PH) return S2ST_ERR_ARG;
  if (adam_pending && !(chunked && fm && ph_fresh)) adam_wait_all(st_);
  if (fm && refresh) {
    if (!ph_fresh) chk(s2st_cast_bf16_rows(P, n_params, PH, n_params, 1, (int)n_params, st_));
    ph_fresh = false;
  }
  return err;
}
// epilogue of every call that leaves nothing for a backward: the tape goes, the first error is returned
int s2st_engine::end_call(int rc) {
  tape.clear();
  return rc ? rc : err;
}

int s2st_engine::forward() {
  const int B = bt.B, S = bt.S, D = bt.D, C = c.enc_dim, Cd = c.dec_dim;
  const int pad = c.conv_k / 2;
  const int T1 = c.text_input ? S : (S + 2 * pad - c.conv_k) / 2 + 1;
  const int T2 = c.text_input ? S : (T1 + 2 * pad - c.conv_k) / 2 + 1;
  if (T2 != bt.E) return S2ST_ERR_SHAPE;
  if (c.text_input && (!bt.src_txt || bt.Ls != S)) return S2ST_ERR_ARG;  // tokens are the encoder input
  const int E = T2;
  const bool tr = bt.training != 0;
  const bool with_loss = bt.tgt != nullptr;
  seed = bt.seed;
  if (tr) ensure_side();  // (also in the dry run that sizes the workspace: same stream set, same allocations)
  dec_overlap = s2st_env_int("S2ST_DEC_OVERLAP", 3);

  // sinusoidal tables come from the host side (cached per dim); conv weight layouts are
  // scratch at the bottom of the workspace
  const float *pe_enc = bt.pe_enc, *pe_dec = bt.pe_dec, *pe_asr = bt.pe_asr, *pe_st = bt.pe_st;
  const bool fm = fast();
  // bf16 copy of the whole parameter arena (292 MB read + 146 MB written: ~0.08 ms)
  if (int rc = params_ready(true)) return rc;
  // transposed weight copies for the backward, made on the second stream (idle during the forward)
  pht_valid = false;
  if (fm && tr && PHT && live()) {
    hipStream_t ts = side_ ? fork_side() : st_;
    // one launch per <= 200 matrices (the table rides in the kernel arguments)
    if (wt_tables.empty()) build_wt_tables();
    for (const s2st_transpose_table& tb : wt_tables) chk(s2st_transpose_bf16_batched(PH, PHT, tb, ts));
    pht_valid = true;
  }
  skws_n = fm ? (long)16 << 20 : 0;
  skws = fm ? alloc(skws_n) : nullptr;
  skws_side = fm && side_allowed ? alloc(skws_n) : skws;  // (by permission, not by existence: the stream is made lazily)
  // stream-K scratch of the persistent GEMM kernel, one per stream (ticket counters zeroed here, before any fork)
  if (fm && tr && sw.use_streamk) {
    float* sk0 = alloc(S2ST_STREAMK_SCRATCH_FLOATS);
    float* sk1 = side_allowed ? alloc(S2ST_STREAMK_SCRATCH_FLOATS) : nullptr;
    if (live()) {
      hipMemsetAsync(sk0, 0, 4096, st_);
      s2st_gemm_streamk_bind(st_, sk0, S2ST_STREAMK_SCRATCH_FLOATS);
      if (sk1 && side_) {
        hipMemsetAsync(sk1, 0, 4096, st_);
        s2st_gemm_streamk_bind(side_, sk1, S2ST_STREAMK_SCRATCH_FLOATS);
      }
    }
  }
  typedef ConvW ConvScratch;
  auto conv_scratch = [&](const ConvP& p, bool need_wd) { return make_conv_scratch(p, need_wd, tr); };
  ConvScratch cs0{}, cs1{};
  std::vector<ConvScratch> cst;  // t2s encoder prenet
  if (c.text_input) {
    for (auto& pc : enc_conv) cst.push_back(conv_scratch(pc, true));
  } else {
    cs0 = conv_scratch(sub[0], false);
    cs1 = conv_scratch(sub[1], true);
  }
  std::vector<ConvScratch> csp;
  {
    // the post-net's weight layouts are first needed at the end of the forward: prepared on the second stream
    // (the data path meets that stream again at the first cross-attention, see cross_attn_block)
    const bool post_on_side = fm && side_ && ev_taps_ && ev_kv_ && live() && sw.hoist_kv && !stop_after_encoder &&
                              c.dec_layers > 0;
    hipStream_t main_st = st_;
    if (post_on_side) st_ = fork_side();
    for (auto& pc : post_conv) csp.push_back(conv_scratch(pc, true));
    st_ = main_st;
  }

  // ---- S2ST_DEC_OVERLAP bit 0: the decoder's front (prenet, positions) and layer 0 up to the cross-attention's query
  //      projection read only prev_output_tokens.  They are issued HERE, on the second stream, and run beside the
  //      encoder layers (behind the optimizer's chunks and the weight transposes, which the stream orders; ahead of the
  //      hoisted K|V projections, which wait for the encoder).  Everything else keeps its place in program order: the
  //      block draws the dropout sites it has behind the encoder's (n_enc_sites are reserved; checked where the block
  //      would run), and its closures, site records and parameter touches are held back and filed at that point, so
  //      tape, segment marks, segment ranges and the site log are what they are without the overlap.  The data path
  //      meets the block at an event of its own (ev_head_), before layer 0's cross-attention.  With the block out of the
  //      way the data path has nothing to do under the hoisted K|V projections any more, so it takes layer 0's itself
  //      (needed at once) and meets the second stream's five at layer 1's cross-attention.
  // (kv_on_side below minus live() -- on hardware.  It goes by the events' creation RESULTS, kv_on_side by their handles:
  //  the emulator's events are null handles, so there the block is issued ahead while all K|V projections stay on the
  //  data-path label; the emulator checks the block's re-ordered issue, the layer-0 / layers-1.. split only runs on a GPU.)
  const bool kv_side_ok = side_ && side_events_ && sw.hoist_kv && !stop_after_encoder;
  const bool dec_early = tr && fm && (dec_overlap & 1) && kv_side_ok && !c.text_input && !c.s2t_mode &&
                         c.dec_layers > 0 && bt.prev && !(dec_spk >= 0 && bt.speaker);
  struct {
    std::vector<std::function<void()>> tape;
    std::vector<s2st_dropout_site> log;
    size_t n_front = 0;          // closures of the prenet and the positions (a segment mark follows them)
    long wm_front = 0, wm_head = 0;
    uint64_t site_first = 0, site_lo = 0, site_hi = 0;  // encoder's first site - 1; the block's sites are (site_lo, site_hi]
    Ten* y = nullptr;
    DecHead head;
  } early;
  auto dec_front = [&](Ten* prev) {
    Ten* h = prev;
    set_ctx("dec.prenet");
    for (int i = 0; i < c.prenet_layers; ++i)
      h = linear(h, prenet[i].w, prenet[i].b, prenet[i].N, prenet[i].K, 1, c.prenet_dropout);
    h = linear(h, prenet.back().w, prenet.back().b, Cd, c.prenet_dim);
    set_ctx("dec.pe");
    return add_pe(h, bt.dec_pos, pe_dec, 1.f, pos_alpha, tr ? c.dropout : 0.f);
  };
  if (dec_early) {
    const int n_enc_sites = (c.dropout > 0.f ? 1 : 0) +
                            c.enc_layers * ((c.attn_dropout > 0.f ? 1 : 0) + (c.dropout > 0.f ? 2 : 0) + (c.act_dropout > 0.f ? 1 : 0));
    hipStream_t main_st = st_;
    const uint64_t site0 = site;
    const long wm0 = param_watermark;
    const size_t t0 = tape.size(), l0 = site_log.size();
    early.site_first = site0;
    early.site_lo = site = site0 + n_enc_sites;
    if (live()) { st_ = fork_side(); dec_early_active = st_ == side_; }  // behind the bf16 parameter copy and the caller's inputs
    Ten* prev = newT(B * D, c.out_dim, const_cast<float*>(bt.prev));
    prev->needs_grad = false;
    early.y = dec_front(prev);
    early.n_front = tape.size() - t0;
    early.wm_front = param_watermark;
    set_ctx("dec.L%d", 0);
    early.head = dec_head(early.y, dec[0], B, D, c.dec_heads, c.dec_pre_ln != 0, bt.tgt_lens);
    early.wm_head = param_watermark;
    early.site_hi = site;
    early.tape.assign(std::make_move_iterator(tape.begin() + t0), std::make_move_iterator(tape.end()));
    tape.resize(t0);
    early.log.assign(site_log.begin() + l0, site_log.end());
    site_log.resize(l0);
    site = site0;
    param_watermark = wm0;
    site_ctx[0] = 0;
    if (live()) hipEventRecord(ev_head_, st_);
    st_ = main_st;
  }

  mark();
  Ten* x = nullptr;
  if (c.text_input) {
    // ---- t2s text front (t2s_transformer.py:85-100): embedding -> conv/BatchNorm/ReLU prenet -> projection ->
    //      x += alpha * positions -> dropout ------------------------------------------------------------------
    Ten* emb = newT(B * E, C);
    touch(enc_embed + (long)c.src_vocab * C);
    if (live()) chk(s2st_embed_fwd((const long*)bt.src_txt, P + enc_embed, emb->d, B * E, C, 1.f, st_));
    const long eoff = enc_embed;
    tape.push_back([=]() {
      if (!emb->g) return;
      if (live()) chk(s2st_embed_bwd((const long*)bt.src_txt, emb->g, G + eoff, B * E, C, 1.f, 1, st_, sw.ordered_sums ? c.src_vocab : 0));
    });
    set_ctx("enc.prenet");
    Ten* pn = text_prenet(emb, B, E, tr, cst);
    Ten* pj = linear(pn, enc_prenet_proj.w, enc_prenet_proj.b, C, C);
    set_ctx("enc.pe");
    x = add_pe(pj, bt.enc_pos, pe_enc, 1.f, enc_pos_alpha, tr ? c.dropout : 0.f);
  } else {
  // ---- encoder front: 2 x (conv k s2 -> GLU), sqrt(C) scale + positions + dropout -------------
  float* xh0 = fm ? nullptr : alloc((long)B * (S + 2 * pad) * c.in_dim, true);
  if (live() && !fm) {
    Split xs{(long)c.in_dim, 0, 0, 0};
    Split ys{(long)c.in_dim, (long)(S + 2 * pad) * c.in_dim, S, 0};
    chk(s2st_copy_rows(bt.src, xs, xh0 + (long)pad * c.in_dim, ys, B * S, c.in_dim, st_));
  }
  const bf16raw* xh0h = fm ? cast_halo(bt.src, B, S, pad, c.in_dim, true) : nullptr;
  Ten* z1 = conv(ConvIn{xh0, nullptr, S, xh0h}, sub[0], B, 2, cs0);
  const int C1 = c.conv_channels / 2;
  // fast mode: the first GLU's result is only read as the second convolution's bf16 operand image: written directly
  // (S2ST_CONVNET_FUSE=0: fp32 image + cast pass)
  const bool glu_img = fm && sw.convnet_fuse && C1 % 4 == 0;
  float* g1h = glu_img ? nullptr : alloc((long)B * (T1 + 2 * pad) * C1, !fm);
  bf16raw* g1img = glu_img ? alloc_h(((long)B * (T1 + 2 * pad) * C1 + 7) / 8 * 8) : nullptr;
  Ten* g1 = glu_img ? glu_to(z1, nullptr, Split{(long)C1, 0, 0, 0}, C1, g1img, B, T1, pad)
                    : glu_to(z1, g1h + (long)pad * C1, Split{(long)C1, (long)(T1 + 2 * pad) * C1, T1, 0}, C1);
  const bf16raw* g1hh = glu_img ? g1img : (fm ? cast_halo(g1h, B, T1, pad, C1) : nullptr);
  Ten* z2 = conv(ConvIn{g1h, g1, T1, g1hh}, sub[1], B, 2, cs1);
  float* x0d = alloc((long)B * E * C);
  Ten* x0 = glu_to(z2, x0d, Split{(long)C, 0, 0, 0}, C);
  set_ctx("enc.pe");
  x = add_pe(x0, bt.enc_pos, pe_enc, c.no_scale_embedding ? 1.f : sqrtf((float)C), -1,
                  tr ? c.dropout : 0.f, enc_spk, E);
  }
  mark();
  // ---- encoder layers, taps -----------------------------------------------------------------
  Ten *tap_asr = nullptr, *tap_st = nullptr;
  for (int i = 0; i < c.enc_layers; ++i) {
    set_ctx("enc.L%d", i);
    x = enc_layer(x, enc[i], B, E);
    if (i == c.tap_asr) tap_asr = x;
    if (i == c.tap_st) tap_st = x;
    if (i % 3 == 2) mark();
  }
  const bool t2s_spk = c.text_input && enc_spk >= 0 && bt.speaker != nullptr;
  Ten* enc_out = has_enc_ln ? layernorm(x, enc_ln, t2s_spk ? nullptr : outs.enc_out) : x;
  if (t2s_spk) {
    // t2s_transformer.py:107-111: x = spk_emb_proj(cat[x, emb.expand(T)]) on EVERY position (padded ones included),
    // after the final layer norm.  The concatenation is materialised so that forward, data gradient and weight
    // gradient are the ordinary linear(); its backward splits the gradient into x's block and the table's rows.
    const int Sd = c.spk_dim;
    Ten* cat = newT(B * E, C + Sd);
    Ten* xin = enc_out;
    touch_spk(enc_spk + (long)c.n_speakers * Sd);
    if (live()) {
      chk(s2st_copy_rows(xin->d, Split{(long)C, 0, 0, 0}, cat->d, Split{(long)(C + Sd), 0, 0, 0}, B * E, C, st_));
      chk(s2st_speaker_fill_cols(spk_tab(enc_spk), (const long*)bt.speaker, cat->d, B, E, C + Sd, C, Sd, st_));
    }
    const long soff = enc_spk;
    tape.push_back([=]() {
      if (!cat->g) return;
      if (!c.spk_frozen && live())
        chk(s2st_speaker_cols_bwd(cat->g, (const long*)bt.speaker, B, E, C + Sd, C, Sd, c.n_speakers, G + soff, st_));
      if (xin->needs_grad) {
        bool acc;
        float* dx = gradbuf(xin, acc);
        if (live()) chk(s2st_split_cols(cat->g, C + Sd, dx, C, B * E, C, acc ? 1 : 0, st_));
      }
    });
    enc_out = linear(cat, enc_spk_proj.w, enc_spk_proj.b, C, C + Sd, 0, 0.f, nullptr, outs.enc_out);
  } else if (!has_enc_ln && outs.enc_out && live())  // post-LN encoder (t2s default): the last layer's output is the result
    hipMemcpyAsync(outs.enc_out, x->d, sizeof(float) * (size_t)x->n(), hipMemcpyDeviceToDevice, st_);
  // (mtl variant / CTC head without the aux ASR decoder: tap 0 is the RAW layer output -- no aux_asr_norm,
  // s2st_transformer_mtl.py:150-153 -- handed out as is for greedy CTC decoding, speech_generator_for_s2st_mtl.py:66-69)
  if (!c.has_asr && tap_asr && outs.tap0 && live())
    hipMemcpyAsync(outs.tap0, tap_asr->d, sizeof(float) * (size_t)tap_asr->n(), hipMemcpyDeviceToDevice, st_);
  if (c.has_asr && tap_asr) tap_asr = layernorm(tap_asr, asr_norm, outs.tap0);
  if (c.has_st && tap_st) tap_st = layernorm(tap_st, st_norm, outs.tap1);
  // the CTC head and the aux text decoders only need the encoder taps: they are issued (below, in tape
  // order) on the second stream behind this event and run next to the mel decoder
  // (t2s feature-level CTC head: it reads the DECODER's output, not an encoder tap -- nothing to overlap, and its
  // backward adds to feature_out's gradient like the post-net's: kept on the data-path stream)
  const bool aux_on_side = side_ && ev_taps_ && live() && sw.overlap_aux && !(c.text_input && c.has_ctc);
  const bool kv_on_side = side_ && ev_taps_ && ev_kv_ && live() && sw.hoist_kv && !stop_after_encoder;
  if (aux_on_side || kv_on_side) hipEventRecord(ev_taps_, st_);
  aux_wait_idx = tape.size();  // the tap layer-norm closures are the last ones pushed so far
  mark();
  if (stop_after_encoder) {  // decode_begin: the AR loop drives the decoder itself
    enc_out_keep = enc_out;
    return err;
  }
  if (c.s2t_mode) return forward_s2t(enc_out, with_loss);
  // The cross-attention K|V projections of every decoder layer only need the encoder output: they are
  // issued here, on the second stream, and run under the prenet and the first self-attention block (their
  // backward -- data gradients into the encoder output, weight gradients -- then runs after the layers').
  std::vector<Ten*> xkv(c.dec_layers, nullptr);
  if (sw.hoist_kv) {
    hipStream_t main_st = st_;
    if (kv_on_side) {
      hipStreamWaitEvent(side_, ev_taps_, 0);
      st_ = side_;
      side_used = true;
    }
    for (int i = 0; i < c.dec_layers; ++i) {
      if (dec_early && i == 0) st_ = main_st;
      xkv[i] = cross_kv(enc_out, dec[i].xa, Cd);
      if (dec_early && i == 0 && kv_on_side) st_ = side_;
    }
    if (kv_on_side) {
      hipEventRecord(ev_kv_, side_);
      st_ = main_st;
      kv_wait_ = !dec_early;  // (dec_early: from layer 1 on, below)
    }
    mark();
  }
  // ---- decoder: prenet (dropout always on), alpha * positions, layers ---------------------------
  tail_lo_idx = tape.size();
  Ten* prev = newT(B * D, c.out_dim, const_cast<float*>(bt.prev));
  prev->needs_grad = false;
  if (dec_spk >= 0 && bt.speaker) {
    // the speaker's row replaces the first input frame (s2st_transformer.py:441-444): a copy of prev_output_tokens
    // with row (b, 0) overwritten; its gradient there is the table's gradient
    Ten* pv = newT(B * D, c.out_dim);
    touch_spk(dec_spk + (long)c.n_speakers * c.out_dim);
    if (live()) {
      hipMemcpyAsync(pv->d, bt.prev, sizeof(float) * (size_t)pv->n(), hipMemcpyDeviceToDevice, st_);
      chk(s2st_speaker_set_rows(spk_tab(dec_spk), (const long*)bt.speaker, pv->d, B, D, c.out_dim, st_));
    }
    pv->needs_grad = tr && !c.spk_frozen;
    const long doff = dec_spk;
    tape.push_back([=]() {
      if (!pv->g || c.spk_frozen) return;
      if (live())
        chk(s2st_speaker_bwd(pv->g, (const long*)bt.speaker, B, D, 1, c.out_dim, c.n_speakers, 0.f, 0, G + doff, st_));
    });
    prev = pv;
  }
  Ten* y = nullptr;
  auto file_early = [&](size_t lo, size_t hi, long wm) {  // closures [lo, hi) of the block issued ahead take their place
    for (size_t k = lo; k < hi; ++k) tape.push_back(std::move(early.tape[k]));
    if (wm > param_watermark) param_watermark = wm;
  };
  if (dec_early) {
    if (site != early.site_lo && !err) {
      // n_enc_sites (above) no longer counts what the encoder's front and layers draw: the block ran with other seeds than
      // in program order.  Loud, never silently another random function; S2ST_DEC_OVERLAP=2 runs without the reservation.
      fprintf(stderr, "[s2st] S2ST_DEC_OVERLAP: %llu dropout sites reserved for the encoder, %llu drawn -- update n_enc_sites "
                      "in forward() (engine_step.cpp)\n", (unsigned long long)(early.site_lo - early.site_first),
              (unsigned long long)(site - early.site_first));
      err = S2ST_ERR_SHAPE;
    }
    site = early.site_hi;
    site_log.insert(site_log.end(), early.log.begin(), early.log.end());
    y = early.y;
    file_early(0, early.n_front, early.wm_front);
    if (live()) wait_traced(st_, ev_head_, "decoder front issued ahead");
  } else {
    y = dec_front(prev);
  }
  mark();
  if (dec_early) file_early(early.n_front, early.tape.size(), early.wm_head);
  float* attn_out = nullptr;
  Ten* tap_dec_t = nullptr;
  // --use-guided-attention-loss: every forward with a loss needs the alignment layer's map, asked for or not (kept in
  // the workspace when the caller gave no buffer), and its backward the term's {sum, N}
  const bool guided = c.guided != 0 && with_loss && c.dec_layers > 0;
  float* guided_map = nullptr;
  float* guided_sum = nullptr;
  if (guided) {
    guided_map = (bt.want_attn && outs.attn) ? outs.attn : alloc((long)B * E * D);
    guided_sum = alloc(2);
  }
  for (int i = 0; i < c.dec_layers; ++i) {
    float* am = (i == c.dec_layers - 1 && bt.want_attn) ? outs.attn : nullptr;
    const bool align = guided && i == c.dec_layers - 1;
    if (align) am = guided_map;
    set_ctx("dec.L%d", i);
    if (dec_early && kv_on_side && i == 1) kv_wait_ = true;
    y = dec_layer(y, enc_out, dec[i], B, D, E, c.dec_heads, c.dec_pre_ln != 0, bt.tgt_lens, am, xkv[i],
                  (dec_early && i == 0) ? &early.head : nullptr, align ? guided_sum : nullptr);
    if (c.has_ctc_tgt && i == c.tap_dec) tap_dec_t = y;  // raw layer output (s2st_transformer_mtl.py:325-327)
    if (i % 2 == 1) mark();
  }
  (void)attn_out;
  // S2ST_DEC_OVERLAP bit 1: the backward's share (backward_segment).  With the projections hoisted, layer 0's query
  // projection is the closure right below its cross-attention's.
  if (tr && kv_side_ok && live() && (dec_overlap & 2) && xattn0_idx > tail_lo_idx) {
    tail_hi_idx = xattn0_idx;
    tail_bwd_on_side = true;
  }
  if (has_dec_ln) y = layernorm(y, dec_ln);
  Ten* feat = linear(y, feat_proj.w, feat_proj.b, c.out_dim, Cd, 0, 0.f, nullptr, outs.feat);
  Ten* eos = linear(y, eos_proj.w, eos_proj.b, 1, Cd, 0, 0.f, nullptr, outs.eos);
  set_ctx("post");
  Ten* post = postnet(feat, B, D, tr, csp, outs.post_feat);
  set_ctx("");
  // ---- mtl variant: CTC over the TARGET text on a decoder layer's output (s2st_loss_mtl.py:171-186: input lengths =
  //      decoder steps, targets = tgt_text incl. EOS) ------------------------------------------------------
  Ten* ctc_tgt_logits = nullptr;
  float *ctc_tgt_per = nullptr, *ctc_tgt_dl = nullptr;
  if (c.has_ctc_tgt && tap_dec_t) {
    ctc_tgt_logits = linear(tap_dec_t, ctc_proj_tgt.w, ctc_proj_tgt.b, c.tgt_vocab, Cd);
    if (with_loss) {
      ctc_tgt_per = alloc(B);
      float* lp = alloc((long)B * D * c.tgt_vocab);
      float* wsd = alloc(s2st_ctc_workspace_floats(B, D, bt.Lt));
      ctc_tgt_dl = tr ? alloc(ctc_tgt_logits->n()) : nullptr;
      if (live())
        chk(s2st_ctc(ctc_tgt_logits->d, (const long*)bt.tgt_txt, bt.Lt, bt.tgt_lens, bt.tgt_txt_lens, B, D, c.tgt_vocab,
                     lp, ctc_tgt_per, ctc_tgt_dl, ctc_tgt_dl ? c.ctc_tgt_weight / B : 0.f, wsd, st_));
    }
  }
  mark();
  // ---- CTC head on tap 0 (ctc_proj lives on the decoder, fed the encoder tap; :458-463) ----------
  hipStream_t main_st = st_;
  aux_lo_idx = tape.size();
  if (aux_on_side) {
    hipStreamWaitEvent(side_, ev_taps_, 0);
    st_ = side_;
    side_used = true;
  }
  Ten* ctc_logits = nullptr;
  if (c.has_ctc && tap_asr && !c.text_input) ctc_logits = linear(tap_asr, ctc_proj.w, ctc_proj.b, c.src_vocab, C);
  // t2s_transformer (criterions/t2s_loss.py:134-144): CTC of the SOURCE TEXT against the decoder's feature_out --
  // log_softmax(ctc_proj(feature_out)) [D, B, V], input lengths = decoder steps, targets = src_text, blank 0
  const bool t2s_ctc = c.text_input && c.has_ctc;
  if (t2s_ctc) ctc_logits = linear(feat, ctc_proj.w, ctc_proj.b, c.src_vocab, c.out_dim);
  const int ctc_T = t2s_ctc ? D : E;
  const int* ctc_ilens = t2s_ctc ? bt.tgt_lens : bt.ctc_in_lens;
  // The CTC sweep (one workgroup per utterance, ~E sequential steps: latency-bound, ~0.4 ms) runs on the
  // second stream next to the aux decoders and the other loss kernels; joined before the loss is finalised.
  float* ctc_per = (with_loss && c.has_ctc) ? alloc(B) : nullptr;
  float *ctc_lp = nullptr, *ctc_ws = nullptr, *ctc_dl = nullptr;
  if (with_loss && c.has_ctc && ctc_logits) {
    ctc_lp = (outs.ctc_lprobs && !t2s_ctc) ? outs.ctc_lprobs : alloc((long)B * ctc_T * c.src_vocab);
    ctc_ws = alloc(s2st_ctc_workspace_floats(B, ctc_T, bt.Ls));
    // training: the CTC gradient w.r.t. the logits comes out of the same alpha/beta sweep as the
    // loss, so it is produced here (per unit of upstream gradient) and only scaled in the backward
    ctc_dl = tr ? alloc(ctc_logits->n()) : nullptr;
    if (live()) {
      hipStream_t cs = aux_on_side ? st_ : fork_side();
      chk(s2st_ctc(ctc_logits->d, (const long*)bt.src_txt, bt.Ls, ctc_ilens, bt.src_txt_lens, B, ctc_T,
                   c.src_vocab, ctc_lp, ctc_per, ctc_dl, ctc_dl ? c.ctc_weight / B : 0.f, ctc_ws, cs));
    }
  }
  // ---- aux text decoders ---------------------------------------------------------------------------
  Ten *asr_logits = nullptr, *st_logits = nullptr;
  if (c.has_asr && tap_asr && bt.prev_src_txt)
    asr_logits = aux_decoder(asr, tap_asr, (const long*)bt.prev_src_txt, bt.src_txt_pos, bt.src_txt_lens, B,
                             bt.Ls, pe_asr, outs.asr_logits);
  if (c.has_st && tap_st && bt.prev_tgt_txt)
    st_logits = aux_decoder(st, tap_st, (const long*)bt.prev_tgt_txt, bt.tgt_txt_pos, bt.tgt_txt_lens, B,
                            bt.Lt, pe_st, outs.st_logits);
  st_ = main_st;
  aux_hi_idx = tape.size();
  aux_bwd_on_side = aux_on_side && tr;
  mark();
  // ---- losses (s2st_loss.py:219-257) -----------------------------------------------------------------
  if (with_loss) {
    float* stats = outs.stats;
    const float nr = (float)bt.ntokens, nf = nr * c.out_dim;
    float* loss_ws = alloc(3L * S2ST_LOSS_ORDERED_FLOATS);
    float* guided_part = guided ? alloc(s2st_guided_attn_blocks(B, E)) : nullptr;
    if (live()) {
      hipMemsetAsync(stats, 0, sizeof(float) * 32, st_);
      // guided-attention term: sum of W (.) alignment over the valid cells and their count (fixed-order sums always)
      if (guided)
        chk(s2st_guided_attn_fwd(guided_map, bt.enc_lens, bt.tgt_lens, B, E, D, c.guided_sigma, guided_part, guided_sum,
                                 nullptr, st_));
      // ordered sums: the loss kernels leave per-workgroup sums, the finalize kernel adds them in workgroup order
      s2st_loss_parts lp{};
      float* ow[3] = {nullptr, nullptr, nullptr};
      if (sw.ordered_sums)
        for (int q = 0; q < 3; ++q) lp.part[q] = ow[q] = loss_ws + (long)q * S2ST_LOSS_ORDERED_FLOATS;
      chk(s2st_mel_loss(feat->d, post->d, eos->d, bt.tgt, bt.tgt_lens, B, D, c.out_dim, c.bce_pos_weight,
                        stats + S2ST_STAT_L1_SUM, 0, 0, 0, nullptr, nullptr, nullptr, st_, ow[0], &lp.nblocks[0]));
      join_side();  // aux logits, CTC per-utterance losses
      if (asr_logits)
        chk(s2st_ls_ce(asr_logits->d, (const long*)bt.src_txt, B * bt.Ls, c.src_vocab, 1, c.label_smoothing,
                       stats + S2ST_STAT_ASR_NLL, nullptr, 0.f, st_, ow[1], &lp.nblocks[1]));
      if (st_logits)
        chk(s2st_ls_ce(st_logits->d, (const long*)bt.tgt_txt, B * bt.Lt, c.tgt_vocab, 1, c.label_smoothing,
                       stats + S2ST_STAT_ST_NLL, nullptr, 0.f, st_, ow[2], &lp.nblocks[2]));
      chk(s2st_loss_finalize(stats, ctc_per, B, nf, nr, c.w_l1, c.w_mse, c.w_eos, c.ctc_weight,
                             c.asr_weight, c.st_weight, c.label_smoothing, c.src_vocab, c.tgt_vocab,
                             (float)bt.src_txt_ntokens, (float)bt.tgt_txt_ntokens, st_, ctc_tgt_per, c.ctc_tgt_weight,
                             sw.ordered_sums ? &lp : nullptr, guided ? guided_sum : nullptr, c.w_attn));
    }
    tape.push_back([=]() {
      // roots of the backward: d loss / d {feat, post, eos, logits}
      const float gs = gscale;
      bool a1, a2, a3;
      float* dfeat = gradbuf(feat, a1);
      float* dpost = gradbuf(post, a2);
      float* deos = gradbuf(eos, a3);
      // post = feat + postnet(feat): the loss kernel adds dpost into dfeat itself, the post-net's last closure then skips
      // its pass over the two (S2ST_CONVNET_FUSE=0: that pass)
      const bool resid = sw.convnet_fuse && !a1 && !a2;
      post->resid_in_loss = resid;
      if (live())
        chk(s2st_mel_loss(feat->d, post->d, eos->d, bt.tgt, bt.tgt_lens, B, D, c.out_dim, c.bce_pos_weight,
                          nullptr, gs * c.w_l1 / nf, gs * c.w_mse / nf, gs * c.w_eos / nr, dfeat, dpost, deos,
                          st_, nullptr, nullptr, resid ? 1 : 0));
      if (ctc_logits) {
        bool a;
        float* dl = gradbuf(ctc_logits, a);
        if (live()) {
          if (ctc_dl) chk(s2st_dropout(ctc_dl, dl, ctc_logits->n(), gs, 0.f, 0, 0, st_));  // dl = gs * ctc_dl
          else
            chk(s2st_ctc(ctc_logits->d, (const long*)bt.src_txt, bt.Ls, ctc_ilens, bt.src_txt_lens, B, ctc_T,
                         c.src_vocab, ctc_lp, ctc_per, dl, gs * c.ctc_weight / B, ctc_ws, st_));
        }
      }
      if (ctc_tgt_logits && ctc_tgt_dl) {
        bool a;
        float* dl = gradbuf(ctc_tgt_logits, a);
        if (live()) chk(s2st_dropout(ctc_tgt_dl, dl, ctc_tgt_logits->n(), gs, 0.f, 0, 0, st_));  // dl = gs * d(ctc_tgt)
      }
      if (asr_logits) {
        bool a;
        float* dl = gradbuf(asr_logits, a);
        if (live())
          chk(s2st_ls_ce(asr_logits->d, (const long*)bt.src_txt, B * bt.Ls, c.src_vocab, 1, c.label_smoothing,
                         nullptr, dl, gs * c.asr_weight / (float)bt.src_txt_ntokens, st_));
      }
      if (st_logits) {
        bool a;
        float* dl = gradbuf(st_logits, a);
        if (live())
          chk(s2st_ls_ce(st_logits->d, (const long*)bt.tgt_txt, B * bt.Lt, c.tgt_vocab, 1, c.label_smoothing,
                         nullptr, dl, gs * c.st_weight / (float)bt.tgt_txt_ntokens, st_));
      }
    });
  }
  if (adam_pending && live()) adam_wait_all(st_);  // (parameters no op of this configuration reads)
  join_side();  // nothing of this forward is left running on the second stream when it returns in st_ order
  mark();
  return err;
}

// s2t_transformer_hubert + s2t_loss (s2t_transformer_me.py:308-330; criterions/s2t_loss.py:80-160): text decoder over the
// encoder output, label-smoothed NLL summed over the non-pad tokens, accuracy counts.  The decoder's tokens ride in the
// batch's source-text slots (the host chose them by --test-type); the dictionary is the TARGET one for both types
// (s2t_transformer_me.py:268-283 builds embedding and output projection from task.target_dictionary).
int s2st_engine::forward_s2t(Ten* enc_out, bool with_loss) {
  const int B = bt.B;
  if (!bt.prev_src_txt || bt.Ls <= 0) return err;  // encoder only (forward_encoder)
  Ten* logits = aux_decoder(s2t, enc_out, (const long*)bt.prev_src_txt, bt.src_txt_pos, bt.src_txt_lens, B, bt.Ls,
                            bt.pe_asr, outs.asr_logits);
  mark();
  if (with_loss && bt.src_txt) {
    float* stats = outs.stats;
    float* loss_ws = alloc(3L * S2ST_LOSS_ORDERED_FLOATS);
    if (live()) {
      hipMemsetAsync(stats, 0, sizeof(float) * 32, st_);
      s2st_loss_parts lp{};
      float* ow = nullptr;
      if (sw.ordered_sums) lp.part[1] = ow = loss_ws + S2ST_LOSS_ORDERED_FLOATS;
      chk(s2st_ls_ce(logits->d, (const long*)bt.src_txt, B * bt.Ls, c.tgt_vocab, 1, c.label_smoothing,
                     stats + S2ST_STAT_ASR_NLL, nullptr, 0.f, st_, ow, &lp.nblocks[1]));
      // (w_asr = 1 over "1 token": the SUM (1 - eps - eps_i) nll + eps_i smooth, eps_i = eps / (V - 1), s2t_loss.py:52-55)
      chk(s2st_loss_finalize(stats, nullptr, B, 1.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, c.label_smoothing, c.tgt_vocab,
                             c.tgt_vocab, 1.f, 1.f, st_, nullptr, 0.f, sw.ordered_sums ? &lp : nullptr));
    }
    tape.push_back([=]() {
      bool a;
      float* dl = gradbuf(logits, a);
      if (live())
        chk(s2st_ls_ce(logits->d, (const long*)bt.src_txt, B * bt.Ls, c.tgt_vocab, 1, c.label_smoothing, nullptr, dl,
                       gscale, st_));
    });
  }
  if (adam_pending && live()) adam_wait_all(st_);
  join_side();
  mark();
  return err;
}

// run tape closures of segment `seg` (0 = last part of the forward)
int s2st_engine::backward_segment(int seg) {
  int ns = n_segments();
  if (seg < 0 || seg >= ns) return S2ST_ERR_ARG;
  if (seg == 0) join_side();  // transposed weights (and anything else the forward left on the side stream)
  size_t hi = marks[ns - seg].tape_idx, lo = marks[ns - seg - 1].tape_idx;
  hipStream_t main_st = st_;
  for (size_t i = hi; i-- > lo;) {
    if (aux_bwd_on_side && live()) {
      // the aux decoders' backward (CTC head + text decoders: many small kernels that only produce
      // the taps' gradients and parameter gradients) runs on the second stream next to the mel
      // decoder's backward; the data path waits for it right before the tap layer norms consume it
      if (i + 1 == aux_hi_idx && st_ == main_st) { flush_wgrad(); flush_lnfold(); st_ = fork_side(); }
      if (i + 1 == aux_lo_idx && st_ != main_st) { flush_wgrad(); flush_lnfold(); hipEventRecord(ev_auxb_, st_); st_ = main_st; }
      if (i + 1 == aux_wait_idx) wait_traced(main_st, ev_auxb_, "aux decoders' backward (tap gradients)");
    }
    if (tail_bwd_on_side && live()) {
      // layer 0 below its cross-attention, positions, prenet (and the speaker row's closure in front of it): parameter
      // gradients only, nothing the data path reads.  No flush_wgrad / flush_lnfold at the switch, unlike the aux section:
      // the invariant is that every input of a queued product or fold was produced EITHER on the data path before the
      // fork_side() below (all data-path closures above the tail ran before it, and none runs until the tail is left) OR on
      // the second stream itself; and the queues are always launched on the second stream, in its order -- from there
      // directly while st_ points at it, through another fork_side() once the data path flushes again.  Nothing queued
      // inside the tail reads what the data path produces after the fork.  The segment-end flush below still runs with
      // st_ on the second stream, so a segment's range is not reported final before its launches are enqueued.
      const bool in_tail = i >= tail_lo_idx && i < tail_hi_idx;
      if (in_tail && st_ == main_st) { st_ = fork_side(); tail_side_ = true; }
      if (!in_tail && tail_side_) { st_ = main_st; tail_side_ = false; }
    }
    tape[i]();
    if (err) break;
  }
  flush_wgrad();  // the segment's gradients are final once its launches are enqueued
  flush_lnfold();
  if (st_ != main_st) {
    if (!tail_side_) hipEventRecord(ev_auxb_, st_);
    st_ = main_st;
  }
  tail_side_ = false;
  // The segment's weight gradients live on the second stream.  A caller that overlaps the gradient
  // all-reduce waits on that stream itself (s2st_engine_side_stream); the data path only joins once,
  // after the last segment, so it never stalls behind the weight-gradient backlog.
  if (seg == ns - 1) join_side();
  return err;
}
