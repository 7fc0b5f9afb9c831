// engine_hifigan.cpp -- the HiFi-GAN generator of --vocoder hifigan: parameters in GEMM-ready layouts and the forward.
#include "engine.h"

using namespace s2st_eng;

// ------------------------------------------------------------------------------------
// HiFi-GAN (fairseq/models/text_to_speech/hifigan.py:109-162): weight-norm folded on the host, conv weights
// [C_out][k][C_in], the transposed convolutions in polyphase form [u][C_out][ceil(k/u)][C_in] (include/s2st_hip.h).
// (the configuration gc and the handles gp: engine.h)
s2st_engine::GanConv s2st_engine::add_gan_conv(const std::string& pre, int cin, int cout, int k, int dil, int phases) {
  GanConv c{0, 0, cin, cout, k, dil};
  c.w = phases > 1 ? add(pre + ".weight", {phases, cout, k, cin}) : add(pre + ".weight", {cout, k, cin});
  c.b = add(pre + ".bias", {cout});
  return c;
}

void s2st_engine::build_params_hifigan() {
  const int C0 = gc.initial_channel;
  gp.pre = add_gan_conv("conv_pre", gc.in_dim, C0, 7, 1);
  for (int i = 0; i < gc.n_ups; ++i) {
    const int u = gc.up_rates[i], k = gc.up_kernels[i];
    gp.ups[i] = add_gan_conv("ups." + std::to_string(i), C0 >> i, C0 >> (i + 1), (k + u - 1) / u, 1, u);
  }
  for (int i = 0; i < gc.n_ups; ++i) {
    const int ch = C0 >> (i + 1);
    for (int j = 0; j < gc.n_kernels; ++j) {
      const std::string pre = "resblocks." + std::to_string(i * gc.n_kernels + j);
      for (int l = 0; l < 3; ++l)
        gp.c1.push_back(add_gan_conv(pre + ".convs1." + std::to_string(l), ch, ch, gc.rb_kernels[j], gc.rb_dilations[j][l]));
      for (int l = 0; l < 3; ++l)
        gp.c2.push_back(add_gan_conv(pre + ".convs2." + std::to_string(l), ch, ch, gc.rb_kernels[j], 1));
    }
  }
  gp.post = add_gan_conv("conv_post", C0 >> gc.n_ups, 1, 7, 1);
}

// length after upsampling layer i of a length-n input: torch's ConvTranspose1d, (n - 1) u - 2 p + k = n u + (k - u - 2 p)
int s2st_engine::gan_extra(int i) const {
  const int u = gc.up_rates[i], k = gc.up_kernels[i];
  return k - u - 2 * ((k - u) / 2);
}
long s2st_engine::hifigan_samples(int T) const {
  if (T <= 0) return 0;
  long n = T;
  for (int i = 0; i < gc.n_ups; ++i) n = n * gc.up_rates[i] + gan_extra(i);
  return n;
}

// one convolution launch (see s2st_hifigan_conv_args); in / img are fp32 images in precise mode, bf16 otherwise
void s2st_engine::gan_conv(const GanConv& cv, const void* in, bool in_f32, int lin, int lout, int nq, int up, const int* off,
                           int la_in, int lb_in, int la_out, int lb_out, const float* resid, float* out, void* img, float slope,
                           int mrf) {
  if (!live()) return;
  s2st_hifigan_conv_args a{};
  a.in = in;
  a.w = c.precise ? (const void*)(P + cv.w) : (const void*)(PH + cv.w);
  a.bias = P + cv.b;
  a.resid = resid; a.out = out; a.img = img; a.frames = gan_frames;
  a.B = bt.B; a.cin = cv.cin; a.lin = lin; a.cout = cv.cout; a.lout = lout; a.nq = nq;
  a.ntap = cv.k; a.dil = cv.dil; a.up = up;
  for (int r = 0; r < up; ++r) a.off[r] = off[r];
  a.la_in = la_in; a.lb_in = lb_in; a.la_out = la_out; a.lb_out = lb_out;
  a.mrf = mrf; a.mrf_div = (float)gc.n_kernels; a.slope = slope;
  a.in_f32 = in_f32 ? 1 : 0; a.precise = c.precise ? 1 : 0;
  chk(s2st_hifigan_conv(a, st_));
}

int s2st_engine::forward_hifigan(const float* mel, const int* frames, int B, int T, float* wave) {
  const bool pr = c.precise != 0;
  if (B <= 0 || T <= 0) return S2ST_ERR_SHAPE;
  bt = s2st_batch{};
  bt.B = B;
  gan_frames = frames;
  constexpr float SLOPE = 0.1f;  // hifigan.py:7 LRELU_SLOPE
  auto img_alloc = [&](long n) -> void* { return pr ? (void*)alloc(n) : (void*)alloc_h(n); };
  const int C0 = gc.initial_channel;
  // conv_pre (80 -> C0, k 7, padding 3), no pre-activation; its only consumer is ups[0] after leaky_relu
  int L = T, la = 1, lb = 0;
  void* x_img = img_alloc((long)B * L * C0);
  {
    const int off = -3;
    gan_conv(gp.pre, mel, true, T, L, L, 1, &off, 1, 0, 1, 0, nullptr, nullptr, x_img, SLOPE);
  }
  float* xs = nullptr;
  for (int i = 0; i < gc.n_ups; ++i) {
    const bool last = i == gc.n_ups - 1;
    const int u = gc.up_rates[i], k = gc.up_kernels[i], p = (k - u) / 2, M = (k + u - 1) / u;
    const int Lo = (L - 1) * u - 2 * p + k, lao = la * u, lbo = lb * u + gan_extra(i), ch = C0 >> (i + 1);
    const long n = (long)B * Lo * ch;
    // the next stage's input image survives this stage; everything else is released at its end
    void* next_img = last ? nullptr : img_alloc(n);
    if (last) xs = alloc(n);
    const long mark = ws_top;
    float* xu = alloc(n);            // upsampled x: residual of every ResBlock's first layer
    void* xu_img = img_alloc(n);     // leaky_relu(x): input of every ResBlock's first conv
    float* xa = alloc(n);            // ResBlock layer outputs (ping-pong)
    float* xb = alloc(n);
    void* xl_img = img_alloc(n);     // leaky_relu of the running ResBlock value
    void* t_img = img_alloc(n);      // leaky_relu(c1(...))
    if (!last) xs = alloc(n);        // the MRF sum
    // ups[i] in polyphase form: phase r reads input rows q + off[r] .. + M - 1 and writes output row q u + r
    int off[8];
    for (int r = 0; r < u; ++r) off[r] = (r + p) / u - M + 1;
    gan_conv(gp.ups[i], x_img, pr, L, Lo, (Lo + u - 1) / u, u, off, la, lb, lao, lbo, nullptr, xu, xu_img, SLOPE);
    for (int j = 0; j < gc.n_kernels; ++j) {
      const float* cur = xu;
      const void* cur_img = xu_img;
      for (int l = 0; l < 3; ++l) {
        const GanConv& c1 = gp.c1[(i * gc.n_kernels + j) * 3 + l];
        const GanConv& c2 = gp.c2[(i * gc.n_kernels + j) * 3 + l];
        const int o1 = -(c1.k * c1.dil - c1.dil) / 2, o2 = -(c2.k - 1) / 2;  // hifigan.py:16 get_padding
        gan_conv(c1, cur_img, pr, Lo, Lo, Lo, 1, &o1, lao, lbo, lao, lbo, nullptr, nullptr, t_img, SLOPE);
        if (l < 2) {
          float* nx = l == 0 ? xa : xb;
          gan_conv(c2, t_img, pr, Lo, Lo, Lo, 1, &o2, lao, lbo, lao, lbo, cur, nx, xl_img, SLOPE);
          cur = nx;
          cur_img = xl_img;
        } else {  // x = c2(...) + x, then the MRF sum: xs = rb0 + rb1 + ..., x = xs / num_kernels (hifigan.py:148-154)
          const int mrf = j == 0 ? 1 : (j == gc.n_kernels - 1 ? 3 : 2);
          const bool fin = j == gc.n_kernels - 1;
          gan_conv(c2, t_img, pr, Lo, Lo, Lo, 1, &o2, lao, lbo, lao, lbo, cur, xs, fin ? next_img : nullptr, SLOPE, mrf);
        }
      }
    }
    ws_top = mark;  // (stream order: the next stage's buffers are only written after this stage's reads)
    if (!last) x_img = next_img;
    L = Lo; la = lao; lb = lbo;
  }
  // leaky_relu (slope 0.01: F.leaky_relu's default, hifigan.py:159) -> conv_post (C -> 1, k 7, padding 3) -> tanh
  if (live()) chk(s2st_hifigan_post(xs, P + gp.post.w, P + gp.post.b, wave, frames, la, lb, B, L, gp.post.cin, 7, 0.01f, st_));
  return err;
}
