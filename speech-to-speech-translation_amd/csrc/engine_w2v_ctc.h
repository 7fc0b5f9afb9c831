// engine_w2v_ctc.h -- a fragment of struct s2st_engine (included INSIDE the struct body by engine.cpp; not a stand-alone
// header): the frozen wav2vec 2.0 CTC recogniser of the ASR-BLEU score: parameters in GEMM-ready layouts and the forward.
  // ------------------------------------------------------------------------------------
  // transformers Wav2Vec2ForCTC with feat_extract_norm = "layer" and do_stable_layer_norm (modeling_wav2vec2.py:
  // Wav2Vec2LayerNormConvLayer, Wav2Vec2FeatureProjection, Wav2Vec2PositionalConvEmbedding, Wav2Vec2EncoderStableLayerNorm,
  // Wav2Vec2EncoderLayerStableLayerNorm, lm_head) under its state_dict names; conv weights [O][k][I], the weight-normed
  // pos_conv as its effective weight [G][E/G][k][E/G] (the host wrapper converts).
  bool is_w2v = false;
  s2st_w2v_ctc_config wc{};
  struct W2vP {
    long conv_w[8], conv_b[8]; LNP conv_ln[8]; LNP ln; LinP proj; long pos_w, pos_b; std::vector<EncLayerP> L; LNP enc_ln;
    LinP lm;
  } wp;

  void build_params_w2v_ctc() {
    int cin = 1;
    for (int i = 0; i < wc.n_conv; ++i) {
      std::string pre = "wav2vec2.feature_extractor.conv_layers." + std::to_string(i);
      wp.conv_w[i] = add(pre + ".conv.weight", {wc.conv_dim[i], wc.conv_k[i], cin});
      wp.conv_b[i] = add(pre + ".conv.bias", {wc.conv_dim[i]});
      wp.conv_ln[i] = add_ln(pre + ".layer_norm", wc.conv_dim[i]);
      cin = wc.conv_dim[i];
    }
    wp.ln = add_ln("wav2vec2.feature_projection.layer_norm", cin);
    wp.proj = add_lin("wav2vec2.feature_projection.projection", wc.embed, cin);
    const int Eg = wc.embed / wc.conv_pos_groups;
    wp.pos_w = add("wav2vec2.encoder.pos_conv_embed.conv.weight", {wc.conv_pos_groups, Eg, wc.conv_pos, Eg});
    wp.pos_b = add("wav2vec2.encoder.pos_conv_embed.conv.bias", {wc.embed});
    for (int l = 0; l < wc.layers; ++l) {
      std::string pre = "wav2vec2.encoder.layers." + std::to_string(l);
      EncLayerP e;
      e.sa = add_self_attn(pre + ".attention", wc.embed);
      e.ln1 = add_ln(pre + ".layer_norm", wc.embed);
      e.fc1 = add_lin(pre + ".feed_forward.intermediate_dense", wc.ffn, wc.embed);
      e.fc2 = add_lin(pre + ".feed_forward.output_dense", wc.embed, wc.ffn);
      e.ln2 = add_ln(pre + ".final_layer_norm", wc.embed);
      wp.L.push_back(e);
    }
    wp.enc_ln = add_ln("wav2vec2.encoder.layer_norm", wc.embed);
    wp.lm = add_lin("lm_head", wc.vocab, wc.embed);
  }

  // _get_feat_extract_output_lengths: floor((n - k) / s) + 1 layer by layer
  int w2v_frames(int n) const {
    for (int i = 0; i < wc.n_conv; ++i) n = n < wc.conv_k[i] ? 0 : (n - wc.conv_k[i]) / wc.conv_stride[i] + 1;
    return n;
  }

  int forward_w2v_ctc(const float* wave, const int* sample_lens, const int* frame_lens, int B, int N, int blank,
                      float* logits_out, int* ids_out, int* counts_out) {
    const bool fm = fast();
    bt = s2st_batch{};
    bt.B = B;
    bt.training = 0;
    bt.enc_lens = frame_lens;
    const int C0 = wc.conv_dim[0];
    int Tin = N < wc.conv_k[0] ? 0 : (N - wc.conv_k[0]) / wc.conv_stride[0] + 1;
    if (Tin <= 0) return S2ST_ERR_SHAPE;
    // the largest tensor (conv0's output, ~102 elements per input sample) must stay countable in 32 bits: the row kernels and
    // the GEMM's tile arithmetic index with int products (about 20 M samples per padded batch for 512 channels)
    if ((long)B * Tin * C0 > 0x7fffffffL || (long)B * N > 0x7fffffffL) return S2ST_ERR_SHAPE;
    // zero_mean_unit_var_norm over each utterance's valid samples, zeros behind them
    float* xn = alloc((long)B * N);
    if (live()) chk(s2st_w2v_wave_norm(wave, sample_lens, xn, B, N, 1e-7f, st_));
    // conv0 (1 -> C0, bias) + LayerNorm(C0) + GELU; fast mode: conv1 only reads the bf16 copy, no fp32 activation exists
    Ten* a = newT(B * Tin, C0, nullptr, !fm);
    if (fm) a->h = alloc_h(a->n());
    if (live())
      chk(s2st_w2v_conv0_ln_gelu(xn, P + wp.conv_w[0], P + wp.conv_b[0], P + wp.conv_ln[0].g, P + wp.conv_ln[0].b, a->d, a->h, B, N,
                                 Tin, C0, wc.conv_k[0], wc.conv_stride[0], 1e-5f, st_));
    // conv_i + bias as GEMMs over the channel-last activations (no padding: windows never cross utterances), then
    // LayerNorm + GELU over every frame's channels; only the last layer's fp32 copy is read (by the projection's norm)
    for (int i = 1; i < wc.n_conv; ++i) {
      const int k = wc.conv_k[i], sd = wc.conv_stride[i], I = wc.conv_dim[i - 1], O = wc.conv_dim[i];
      const int Tout = Tin < k ? 0 : (Tin - k) / sd + 1;
      if (Tout <= 0) return S2ST_ERR_SHAPE;
      const bool last = i == wc.n_conv - 1;
      Ten* z = newT(B * Tout, O);
      Ten* y = (fm && !last) ? newT(B * Tout, O, nullptr, false) : newT(B * Tout, O, z->d);  // (fp32: normalised in place)
      if (fm) y->h = alloc_h(y->n());
      if (live()) {
        GemmArgs g{};
        g.A = fm ? gemm_rowmajor(a->h, (long)sd * I) : gemm_rowmajor(a->d, (long)sd * I);
        g.A.sp.per = Tout; g.A.sp.bs = (long)Tin * I;
        g.B = fm ? gemm_rowmajor(PH + wp.conv_w[i], (long)k * I) : gemm_rowmajor(P + wp.conv_w[i], (long)k * I);
        g.C = gemm_out(z->d, O);
        g.ep = gemm_epi_default();
        g.ep.bias = P + wp.conv_b[i];
        g.M = B * Tout; g.N = O; g.K = k * I; g.batch = 1; g.zdiv = 1; g.precise = c.precise;
        chk(s2st_gemm(g, st_));
        chk(s2st_w2v_ln_gelu_rows(z->d, P + wp.conv_ln[i].g, P + wp.conv_ln[i].b, (fm && !last) ? nullptr : y->d, y->h, B * Tout, O,
                                  1e-5f, st_));
      }
      a = y;
      Tin = Tout;
    }
    const int T = Tin, E = wc.embed, G = wc.conv_pos_groups, Eg = E / G, kp = wc.conv_pos, V = wc.vocab;
    Ten* x = linear(layernorm(a, wp.ln, nullptr, true), wp.proj.w, wp.proj.b, E, wp.proj.K);
    // frames at or past the length -> 0; x += gelu(pos_conv(x)) with SamePad, the G groups as ONE batched product
    const int pad = kp / 2, Tp = T + kp;
    float* img = fm ? nullptr : alloc((long)G * B * Tp * Eg, true);
    bf16raw* imgh = fm ? alloc_h((long)G * B * Tp * Eg) : nullptr;
    if (fm && live()) hipMemsetAsync(imgh, 0, sizeof(bf16raw) * (size_t)G * B * Tp * Eg, st_);
    Ten* x2 = newT(B * T, E);
    if (live()) {
      chk(s2st_posconv_prep(x->d, frame_lens, img, imgh, B, T, E, G, pad, Tp, st_));
      GemmArgs g{};
      g.A = fm ? gemm_rowmajor(imgh, Eg) : gemm_rowmajor(img, Eg);
      g.A.sp.per = T; g.A.sp.bs = (long)Tp * Eg;
      g.B = fm ? gemm_rowmajor(PH + wp.pos_w, (long)kp * Eg) : gemm_rowmajor(P + wp.pos_w, (long)kp * Eg);
      g.C = gemm_out(x2->d, E);
      g.ep = gemm_epi_default();
      g.ep.bias = P + wp.pos_b;
      g.ep.act = 2;
      g.ep.resid = x->d;
      g.M = B * T; g.N = Eg; g.K = kp * Eg; g.batch = G; g.zdiv = 1; g.precise = c.precise;
      g.A.zo = (long)B * Tp * Eg; g.B.zo = (long)Eg * kp * Eg; g.C.zo = Eg; g.ep.bias_zo = Eg;
      chk(s2st_gemm(g, st_));
    }
    // pre-LN layers: x += attn(LN(x)); x += fc2(gelu(fc1(LN(x)))); the normalised activations only feed GEMMs
    Ten* y = x2;
    for (int l = 0; l < wc.layers; ++l) {
      const EncLayerP& L = wp.L[l];
      y = self_attn_block(layernorm(y, L.ln1, nullptr, true), L.sa, B, T, wc.heads, frame_lens, 0, y);
      y = ffn_block(layernorm(y, L.ln2, nullptr, true), L.fc1, L.fc2, y);
    }
    y = layernorm(y, wp.enc_ln, nullptr, true);
    Ten* lg = linear(y, wp.lm.w, wp.lm.b, V, E, 0, 0.f, nullptr, logits_out);
    if (ids_out && live()) chk(s2st_w2v_ctc_greedy(lg->d, frame_lens, ids_out, counts_out, B, T, V, blank, st_));
    return err;
  }
