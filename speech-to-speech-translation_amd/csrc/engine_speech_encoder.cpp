// engine_speech_encoder.cpp -- the two frozen wav2vec 2.0-family speech encoders -- the HuBERT front end of config 4 and
// the wav2vec 2.0 CTC recogniser of the ASR-BLEU score: parameters in GEMM-ready layouts and the one forward.
#include "engine.h"

using namespace s2st_eng;

// ------------------------------------------------------------------------------------
// Both are: a strided conv stack over the waveform, LayerNorm + projection, a grouped weight-normed positional
// convolution, a transformer encoder, a final LayerNorm.  They differ in five places, all decided by the variant:
//                GroupNormPostLN (HuBERT base)                     LayerNormPreLN (wav2vec 2.0 large + CTC head)
//   input        raw waveform                                      zero-mean / unit-variance per utterance first
//   conv 0       GroupNorm over time + GELU (a stats scratch)      bias, LayerNorm over channels + GELU
//   conv i >= 1  GEMM, GELU in the epilogue, no bias               GEMM + bias, then LayerNorm + GELU over the rows
//   layers       enc_ln first, then post-LN layers                 pre-LN layers, then enc_ln
//   tail         the last LayerNorm writes the features            lm_head, then the greedy CTC collapse
// GroupNormPostLN: fairseq HubertModel.extract_features, eval, mask=False (fairseq/models/hubert/hubert.py:412-461,
// 518-534; wav2vec2.py:736-905) under its state_dict names.  LayerNormPreLN: transformers Wav2Vec2ForCTC with
// feat_extract_norm = "layer" and do_stable_layer_norm (modeling_wav2vec2.py: Wav2Vec2LayerNormConvLayer,
// Wav2Vec2FeatureProjection, Wav2Vec2PositionalConvEmbedding, Wav2Vec2EncoderStableLayerNorm, lm_head) under its names.
// Conv weights are stored [O][k][I], the weight-normed pos_conv as its effective weight [G][E/G][k][E/G]; the host
// wrapper converts from the reference layouts.
// (SpeechVariant, the configuration sc and the handles sp: engine.h)

// the variants' state_dict names: checkpoints and the host wrappers' tables depend on names, order and shapes
const s2st_engine::SpeechNames& s2st_engine::speech_names(SpeechVariant v) {
  static const SpeechNames names[2] = {
      {"feature_extractor.conv_layers.", ".0", ".2", "layer_norm", "post_extract_proj", "encoder.pos_conv.0", "encoder.layers.",
       ".self_attn", ".self_attn_layer_norm", ".fc1", ".fc2", "encoder.layer_norm"},
      {"wav2vec2.feature_extractor.conv_layers.", ".conv", ".layer_norm", "wav2vec2.feature_projection.layer_norm",
       "wav2vec2.feature_projection.projection", "wav2vec2.encoder.pos_conv_embed.conv", "wav2vec2.encoder.layers.",
       ".attention", ".layer_norm", ".feed_forward.intermediate_dense", ".feed_forward.output_dense",
       "wav2vec2.encoder.layer_norm"}};
  return names[v == SpeechVariant::LayerNormPreLN];
}

void s2st_engine::build_params_speech() {
  const bool pre_ln = sv == SpeechVariant::LayerNormPreLN;
  const SpeechNames& nm = speech_names(sv);
  int cin = 1;
  for (int i = 0; i < sc.n_conv; ++i) {
    const std::string pre = nm.conv + std::to_string(i);
    sp.conv_w[i] = add(pre + nm.conv_w + ".weight", {sc.conv_dim[i], sc.conv_k[i], cin});
    if (pre_ln) sp.conv_b[i] = add(pre + nm.conv_w + ".bias", {sc.conv_dim[i]});
    if (pre_ln || i == 0) sp.conv_ln[i] = add_ln(pre + nm.conv_norm, sc.conv_dim[i]);
    cin = sc.conv_dim[i];
  }
  sp.ln = add_ln(nm.ln, cin);
  sp.proj = add_lin(nm.proj, sc.embed, cin);
  const int Eg = sc.embed / sc.conv_pos_groups;
  sp.pos_w = add(std::string(nm.pos) + ".weight", {sc.conv_pos_groups, Eg, sc.conv_pos, Eg});
  sp.pos_b = add(std::string(nm.pos) + ".bias", {sc.embed});
  for (int l = 0; l < sc.layers; ++l) {
    const std::string pre = nm.layers + std::to_string(l);
    EncLayerP e;
    e.sa = add_self_attn(pre + nm.attn, sc.embed);
    e.ln1 = add_ln(pre + nm.ln1, sc.embed);
    e.fc1 = add_lin(pre + nm.fc1, sc.ffn, sc.embed);
    e.fc2 = add_lin(pre + nm.fc2, sc.embed, sc.ffn);
    e.ln2 = add_ln(pre + ".final_layer_norm", sc.embed);
    sp.L.push_back(e);
  }
  sp.enc_ln = add_ln(nm.enc_ln, sc.embed);
  if (pre_ln) sp.lm = add_lin("lm_head", sc.vocab, sc.embed);
}

// frames of n samples: floor((n - k) / s) + 1 layer by layer (_get_feat_extract_output_lengths); 0 when too short
int s2st_engine::speech_frames(int n) const {
  for (int i = 0; i < sc.n_conv; ++i) n = n < sc.conv_k[i] ? 0 : (n - sc.conv_k[i]) / sc.conv_stride[i] + 1;
  return n;
}

// GroupNormPostLN: out = the features [B][T][embed]; sample_lens, blank, ids_out and counts_out are not read.
// LayerNormPreLN: out = the logits [B][T][vocab].
int s2st_engine::forward_speech(const float* wave, const int* sample_lens, const int* frame_lens, int B, int N, float* out, int blank,
                                int* ids_out, int* counts_out) {
  const bool fm = fast(), pre_ln = sv == SpeechVariant::LayerNormPreLN;
  bt = s2st_batch{};
  bt.B = B;
  bt.training = 0;
  bt.enc_lens = frame_lens;
  const int C0 = sc.conv_dim[0];
  int Tin = N < sc.conv_k[0] ? 0 : (N - sc.conv_k[0]) / sc.conv_stride[0] + 1;
  if (Tin <= 0) return S2ST_ERR_SHAPE;
  // the largest tensor (conv0's output, ~102 elements per input sample) must stay countable in 32 bits: the row kernels and
  // the GEMM's tile arithmetic index with int products (about 20 M samples per padded batch for 512 channels)
  if ((long)B * Tin * C0 > 0x7fffffffL || (long)B * N > 0x7fffffffL) return S2ST_ERR_SHAPE;
  // [1 input] LayerNormPreLN: zero_mean_unit_var_norm over each utterance's valid samples, zeros behind them
  float* xn = pre_ln ? alloc((long)B * N) : nullptr;
  if (pre_ln && live()) chk(s2st_w2v_wave_norm(wave, sample_lens, xn, B, N, 1e-7f, st_));
  // [2 conv 0] (1 -> C0) + GroupNorm(C0, C0) over ALL Tin frames of the padded batch + GELU, or (bias) + LayerNorm(C0) +
  // GELU; fast mode: conv1 only reads the bf16 copy, no fp32 activation is allocated or written
  Ten* a = newT(B * Tin, C0, nullptr, !fm);
  float* stats = pre_ln ? nullptr : alloc(s2st_hubert_conv0_stats_floats(B, Tin, C0));
  if (fm) a->h = alloc_h(a->n());
  if (live())
    chk(pre_ln ? s2st_w2v_conv0_ln_gelu(xn, P + sp.conv_w[0], P + sp.conv_b[0], P + sp.conv_ln[0].g, P + sp.conv_ln[0].b, a->d,
                                        a->h, B, N, Tin, C0, sc.conv_k[0], sc.conv_stride[0], 1e-5f, st_)
               : s2st_hubert_conv0_gn_gelu(wave, P + sp.conv_w[0], P + sp.conv_ln[0].g, P + sp.conv_ln[0].b, a->d, a->h, stats,
                                           B, N, Tin, C0, sc.conv_k[0], sc.conv_stride[0], 1e-5f, st_));
  // [3 conv i >= 1] GEMMs over the channel-last activations (no padding: windows never cross utterances): y = the product
  // with GELU in the epilogue, or z = the product + bias and y = GELU(LayerNorm(z)) over every frame's channels (fp32:
  // normalised in place; only the last layer's fp32 copy is read, by the projection's norm)
  for (int i = 1; i < sc.n_conv; ++i) {
    const int k = sc.conv_k[i], sd = sc.conv_stride[i], I = sc.conv_dim[i - 1], O = sc.conv_dim[i];
    const int Tout = Tin < k ? 0 : (Tin - k) / sd + 1;
    if (Tout <= 0) return S2ST_ERR_SHAPE;
    const bool y_h_only = fm && i < sc.n_conv - 1;
    Ten* z = newT(B * Tout, O);
    Ten* y = !pre_ln ? z : y_h_only ? newT(B * Tout, O, nullptr, false) : newT(B * Tout, O, z->d);
    if (fm) y->h = alloc_h(y->n());
    if (live()) {
      GemmArgs g{};
      g.A = fm ? gemm_rowmajor(a->h, (long)sd * I) : gemm_rowmajor(a->d, (long)sd * I);
      g.A.sp.per = Tout; g.A.sp.bs = (long)Tin * I;
      g.B = fm ? gemm_rowmajor(PH + sp.conv_w[i], (long)k * I) : gemm_rowmajor(P + sp.conv_w[i], (long)k * I);
      g.C = gemm_out(z->d, O);
      g.ep = gemm_epi_default();
      if (pre_ln) {
        g.ep.bias = P + sp.conv_b[i];
      } else {
        g.C.h = y->h;
        g.ep.act = 2;
      }
      g.M = B * Tout; g.N = O; g.K = k * I; g.batch = 1; g.zdiv = 1; g.precise = c.precise;
      chk(s2st_gemm(g, st_));
      if (pre_ln)
        chk(s2st_w2v_ln_gelu_rows(z->d, P + sp.conv_ln[i].g, P + sp.conv_ln[i].b, y_h_only ? nullptr : y->d, y->h, B * Tout, O,
                                  1e-5f, st_));
    }
    a = y;
    Tin = Tout;
  }
  const int T = Tin, E = sc.embed, G = sc.conv_pos_groups, Eg = E / G, kp = sc.conv_pos;
  // (pre-LN: the normalised activations only feed GEMMs)
  Ten* x = linear(layernorm(a, sp.ln, nullptr, pre_ln), sp.proj.w, sp.proj.b, E, sp.proj.K);
  // frames at or past the length -> 0 (wav2vec2.py:870-871); x += gelu(pos_conv(x)) with SamePad (:873-875)
  const int pad = kp / 2, Tp = T + kp;
  float* img = fm ? nullptr : alloc((long)G * B * Tp * Eg, true);
  bf16raw* imgh = fm ? alloc_h((long)G * B * Tp * Eg) : nullptr;
  if (fm && live()) hipMemsetAsync(imgh, 0, sizeof(bf16raw) * (size_t)G * B * Tp * Eg, st_);
  Ten* x2 = newT(B * T, E);
  if (live()) {
    chk(s2st_posconv_prep(x->d, frame_lens, img, imgh, B, T, E, G, pad, Tp, st_));
    // the G groups as ONE batched product (one launch per group: 16 launches of 150 tiles each -- a third of the CUs --
    // took 515 us of HuBERT's 5.8 ms forward): group z reads its image and its [Eg][kp * Eg] weights, writes columns
    // [z Eg, (z + 1) Eg) of x2 (bias and residual follow the columns)
    GemmArgs g{};
    g.A = fm ? gemm_rowmajor(imgh, Eg) : gemm_rowmajor(img, Eg);
    g.A.sp.per = T; g.A.sp.bs = (long)Tp * Eg;
    g.B = fm ? gemm_rowmajor(PH + sp.pos_w, (long)kp * Eg) : gemm_rowmajor(P + sp.pos_w, (long)kp * Eg);
    g.C = gemm_out(x2->d, E);
    g.ep = gemm_epi_default();
    g.ep.bias = P + sp.pos_b;
    g.ep.act = 2;
    g.ep.resid = x->d;
    g.M = B * T; g.N = Eg; g.K = kp * Eg; g.batch = G; g.zdiv = 1; g.precise = c.precise;
    g.A.zo = (long)B * Tp * Eg; g.B.zo = (long)Eg * kp * Eg; g.C.zo = Eg; g.ep.bias_zo = Eg;
    chk(s2st_gemm(g, st_));
  }
  // [4 layers] post-LN: x = LN(x + attn(x)); x = LN(x + fc2(gelu(fc1(x)))), the last one into `out`.
  // pre-LN: x += attn(LN(x)); x += fc2(gelu(fc1(LN(x)))); the normalised activations only feed GEMMs
  Ten* y = pre_ln ? x2 : layernorm(x2, sp.enc_ln);
  for (int l = 0; l < sc.layers; ++l) {
    const EncLayerP& L = sp.L[l];
    if (pre_ln) {
      y = self_attn_block(layernorm(y, L.ln1, nullptr, true), L.sa, B, T, sc.heads, frame_lens, 0, y);
      y = ffn_block(layernorm(y, L.ln2, nullptr, true), L.fc1, L.fc2, y);
    } else {
      y = layernorm(self_attn_block(y, L.sa, B, T, sc.heads, frame_lens, 0, y), L.ln1);
      y = layernorm(ffn_block(y, L.fc1, L.fc2, y), L.ln2, l == sc.layers - 1 ? out : nullptr);
    }
  }
  // [5 tail]
  if (pre_ln) {
    y = layernorm(y, sp.enc_ln, nullptr, true);
    Ten* lg = linear(y, sp.lm.w, sp.lm.b, sc.vocab, E, 0, 0.f, nullptr, out);
    if (ids_out && live()) chk(s2st_w2v_ctc_greedy(lg->d, frame_lens, ids_out, counts_out, B, T, sc.vocab, blank, st_));
  }
  return err;
}
