// Kernels of the HiFi-GAN generator (--vocoder hifigan): the stride-1 dilated convolutions of the multi-receptive-field
// ResBlocks and conv_pre as implicit GEMMs, the strided transposed convolutions in polyphase form on the same kernel, and
// conv_post + tanh as a per-sample reduction.  Forward only, frozen weights.
//
// Reference call sites replaced: fairseq/models/text_to_speech/hifigan.py:96-104 (ResBlock.forward: leaky_relu -> c1 ->
// leaky_relu -> c2 -> residual add), :140-158 (Generator.forward: conv_pre, leaky_relu -> ups[i], the MRF sum
// xs = rb0 + rb1 + ... then / num_kernels), :159-162 (leaky_relu with the default slope 0.01 -> conv_post -> tanh).
//
// Layouts.  Activations are channel-last images [B][L][C] with L the batch's longest length at that stage; rows at or past
// an utterance's own length are exact zeros in every image (written so by every epilogue).  The convolutions read their
// input rows through the utterance's length -- a row outside [0, len) is taken as zero when it is staged -- so the
// images carry no halo rows and a batched utterance sees the zero padding a one-utterance run of the reference sees.
// Weights are [phase][C_out][taps][C_in] (the GEMM's N x K, K contiguous).
//
// One workgroup owns HG_TM output rows of ONE utterance (and of one output phase) x HG_TN output channels.  Per chunk of
// 32 input channels (the MFMA's K; channel counts that are not a multiple of 32 -- conv_pre's 80, narrow stages -- are
// zero-padded in LDS) it stages the tile's rows plus their (taps - 1) * dilation halo rows ONCE and reads them for every
// tap: the input crosses HBM once per convolution, not once per tap.  Weight fragments are read straight from global memory
// (they are small and stay in L2).  An output element's accumulation order is (chunk, tap, MFMA K) whatever the batch or
// the tile, so a batched call is bit-identical to one call per utterance.
//
// Fast mode: bf16 images and weights, bf16 MFMA with fp32 accumulation, fp32 residual stream.  Precise mode (bf16x3):
// fp32 images and weights, each split hi + lo at the fragment, three MFMAs per product (hi*hi + hi*lo + lo*hi).
#include <type_traits>
#include "s2st_ops.h"
#include "s2st_prof.h"

namespace {

constexpr int HG_TM = 128;                // output rows (of one phase) per workgroup
constexpr int HG_TN = 64;                 // output channels per workgroup
constexpr int HG_KC = 32;                 // input channels per LDS chunk (= MFMA K)
constexpr int HG_HALO = 64;               // max (taps - 1) * dilation
constexpr int HG_ROWS = HG_TM + HG_HALO;  // staged rows per chunk

__device__ __forceinline__ int hg_len(const int* frames, int b, int la, int lb) {
  const int f = frames[b];
  return f > 0 ? f * la + lb : 0;
}

__device__ __forceinline__ bf16x8 hg_join(uint2 a, uint2 b) {
  union { uint4 u; bf16x8 v; } c;
  c.u = make_uint4(a.x, a.y, b.x, b.y);
  return c.v;
}

// 8 consecutive elements -> bf16 fragment (fast) or hi / lo fragments (precise)
template <bool PREC>
__device__ __forceinline__ void hg_frag(const void* p, bf16x8& hi, bf16x8& lo) {
  if (PREC) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    uint2 h0, l0, h1, l1;
    split_bf16x4(a.x, a.y, a.z, a.w, h0, l0);
    split_bf16x4(b.x, b.y, b.z, b.w, h1, l1);
    hi = hg_join(h0, h1);
    lo = hg_join(l0, l1);
  } else {
    union { uint4 u; bf16x8 v; } c;
    c.u = *reinterpret_cast<const uint4*>(p);
    hi = c.v;
  }
}

// y[b][q u + r][o] = epilogue(bias[o] + sum_{c, j} x[b][q + off[r] + j dil][c] * w[r][o][j][c]), q < nq
// (u = 1, off = -pad: a stride-1 conv; u > 1: phase r of a transposed conv)
struct HgConvArgs {
  const void* in;       // [B][lin][cin], fp32 (IN32) or bf16
  const void* w;        // [up][cout][ntap][cin], fp32 (PREC) or bf16
  const float* bias;    // [cout]
  const float* resid;   // optional [B][lout][cout] fp32: added after the bias
  float* out;           // optional [B][lout][cout] fp32 (also the MRF accumulator: mrf 2 / 3 read it first)
  void* img;            // optional [B][lout][cout] leaky_relu(y, slope), fp32 (PREC) or bf16
  const int* frames;    // [B] mel frames; a stage's length is frames * la + lb (0 for an empty utterance)
  int cin, lin, cout, lout, nq;
  int ntap, dil, up, off[8];
  int la_in, lb_in, la_out, lb_out;
  int mrf;              // 0: y; 1: out = y; 2: out += y; 3: out = (out + y) / mrf_div
  float mrf_div, slope;
};

// RB: 16-row blocks per wave -- 4: 2 x 2 waves of 64 rows x 32 channels; 2: 4 x 1 waves of 32 rows x 32 channels
// (cout <= 32, where a second column of waves would have nothing to do)
template <bool PREC, bool IN32, int RB>
__global__ __launch_bounds__(256) void hifigan_conv_kernel(HgConvArgs a) {
  static_assert(!PREC || IN32, "precise mode reads fp32 images");
  using act_t = typename std::conditional<PREC, float, bf16raw>::type;
  constexpr int LD = PREC ? HG_KC + 4 : HG_KC + 8;  // LDS row pitch (elements): 144 / 80 bytes
  __shared__ __attribute__((aligned(16))) act_t xs[HG_ROWS * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z / a.up, r = blockIdx.z - b * a.up;
  const int q0 = blockIdx.x * HG_TM, n0 = blockIdx.y * HG_TN;
  const int len_in = min(hg_len(a.frames, b, a.la_in, a.lb_in), a.lin), len_out = min(hg_len(a.frames, b, a.la_out, a.lb_out), a.lout);
  const int row_w = (RB == 4 ? (wave >> 1) : wave) * RB * 16;
  const int col_w = n0 + (RB == 4 ? (wave & 1) * 32 : 0);
  const int rbase = q0 + a.off[r];
  const int nrows = HG_TM + (a.ntap - 1) * a.dil;
  // nothing of this workgroup's rows is inside the utterance: zeros only (no loads)
  const bool any = (long)q0 * a.up + r < len_out;
  const bool wave_on = any && col_w < a.cout && col_w < n0 + HG_TN;
  f32x4 acc[RB][2];
#pragma unroll
  for (int i = 0; i < RB; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long in_b = (long)b * a.lin * a.cin;
  const long w_r = (long)r * a.cout * a.ntap * a.cin;
  for (int c0 = 0; any && c0 < a.cin; c0 += HG_KC) {
    __syncthreads();
    // stage rows [rbase, rbase + nrows) x channels [c0, c0 + 32): 8 channels (16 bytes of bf16 / 2 x 16 of fp32) per item
    for (int i = tid; i < nrows * (HG_KC / 8); i += 256) {
      const int rr = i >> 2, cv = (i & 3) * 8;
      const int ri = rbase + rr, c = c0 + cv;
      act_t* d = xs + rr * LD + cv;
      const bool ok = ri >= 0 && ri < len_in && c < a.cin;
      if (IN32) {
        float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
        if (ok) {
          const float* s = reinterpret_cast<const float*>(a.in) + in_b + (long)ri * a.cin + c;
          v0 = reinterpret_cast<const float4*>(s)[0];
          v1 = reinterpret_cast<const float4*>(s)[1];
        }
        if (PREC) {
          reinterpret_cast<float4*>(d)[0] = v0;
          reinterpret_cast<float4*>(d)[1] = v1;
        } else {
          const uint2 h0 = pack_bf16x4(v0.x, v0.y, v0.z, v0.w), h1 = pack_bf16x4(v1.x, v1.y, v1.z, v1.w);
          *reinterpret_cast<uint4*>(d) = make_uint4(h0.x, h0.y, h1.x, h1.y);
        }
      } else {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (ok) v = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16raw*>(a.in) + in_b + (long)ri * a.cin + c);
        *reinterpret_cast<uint4*>(d) = v;
      }
    }
    __syncthreads();
    if (!wave_on) continue;
    const int kc = c0 + 8 * (lane >> 4);  // this lane's 8 channels of the chunk
    for (int j = 0; j < a.ntap; ++j) {
      bf16x8 bh[2], bl[2];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb) {
        const int o = col_w + cb * 16 + (lane & 15);
        if (o < a.cout && kc < a.cin) {
          hg_frag<PREC>(reinterpret_cast<const act_t*>(a.w) + w_r + ((long)o * a.ntap + j) * a.cin + kc, bh[cb], bl[cb]);
        } else {
          bh[cb] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
          bl[cb] = bh[cb];
        }
      }
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        bf16x8 ah, al;
        hg_frag<PREC>(xs + (row_w + rb * 16 + (lane & 15) + j * a.dil) * LD + 8 * (lane >> 4), ah, al);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          if (PREC) {
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[cb], acc[rb][cb], 0, 0, 0);
            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[cb], acc[rb][cb], 0, 0, 0);
          }
          acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[cb], acc[rb][cb], 0, 0, 0);
        }
      }
    }
  }
  // epilogue: accumulator element (rb, cb, e) is row row_w + 16 rb + 4 (lane >> 4) + e, channel col_w + 16 cb + (lane & 15)
  if (col_w >= a.cout || col_w >= n0 + HG_TN) return;
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    const int o = col_w + cb * 16 + (lane & 15);
    if (o >= a.cout) continue;
    const float bias = a.bias[o];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int q = q0 + row_w + rb * 16 + 4 * (lane >> 4) + e;
        if (q >= a.nq) continue;
        const int s = q * a.up + r;
        if (s >= a.lout) continue;
        const long idx = ((long)b * a.lout + s) * a.cout + o;
        float v = 0.f;  // rows past the utterance: exact zeros in every output
        if (s < len_out) {
          v = acc[rb][cb][e] + bias;
          if (a.resid) v += a.resid[idx];
          if (a.mrf == 2) v = a.out[idx] + v;
          else if (a.mrf == 3) v = (a.out[idx] + v) / a.mrf_div;
        }
        if (a.out) a.out[idx] = v;
        if (a.img) {
          const float l = v > 0.f ? v : v * a.slope;
          if (PREC) reinterpret_cast<float*>(a.img)[idx] = l;
          else reinterpret_cast<bf16raw*>(a.img)[idx] = (bf16raw)(pack_bf16x4(l, 0.f, 0.f, 0.f).x & 0xffffu);
        }
      }
  }
}

// wave[b][t] = tanh(bias + sum_{j < k, c} w[j][c] * leaky_relu(x[b][t - k / 2 + j][c], slope)), zero for t >= len
// (conv_post: C -> 1, "same" padding).  One thread per sample, taps then channels in order.
__global__ __launch_bounds__(256) void hifigan_post_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ bias, float* __restrict__ wave,
                                                           const int* __restrict__ frames, int la, int lb, int L, int C,
                                                           int k, float slope) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= L) return;
  const int len = min(hg_len(frames, b, la, lb), L);
  float acc = 0.f;
  if (t < len) {
    for (int j = 0; j < k; ++j) {
      const int ri = t - k / 2 + j;
      if (ri < 0 || ri >= len) continue;
      const float* xr = x + ((long)b * L + ri) * C;
      const float* wr = w + (long)j * C;
      for (int c = 0; c < C; c += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + c), wv = *reinterpret_cast<const float4*>(wr + c);
        acc = fmaf(wv.x, xv.x > 0.f ? xv.x : xv.x * slope, acc);
        acc = fmaf(wv.y, xv.y > 0.f ? xv.y : xv.y * slope, acc);
        acc = fmaf(wv.z, xv.z > 0.f ? xv.z : xv.z * slope, acc);
        acc = fmaf(wv.w, xv.w > 0.f ? xv.w : xv.w * slope, acc);
      }
    }
    acc = tanhf(acc + bias[0]);
  }
  wave[(long)b * L + t] = acc;
}

}  // namespace

int s2st_hifigan_conv(const s2st_hifigan_conv_args& c, hipStream_t st) {
  if (c.up < 1 || c.up > 8 || c.ntap < 1 || (c.ntap - 1) * c.dil > HG_HALO || c.dil < 1 || c.cin % 8 || c.cin < 8 ||
      c.cout < 1 || (c.mrf > 0 && !c.out) || (c.precise && !c.in_f32))
    return S2ST_ERR_SHAPE;
  if (c.B <= 0 || c.nq <= 0) return 0;
  HgConvArgs a;
  a.in = c.in; a.w = c.w; a.bias = c.bias; a.resid = c.resid; a.out = c.out; a.img = c.img; a.frames = c.frames;
  a.cin = c.cin; a.lin = c.lin; a.cout = c.cout; a.lout = c.lout; a.nq = c.nq;
  a.ntap = c.ntap; a.dil = c.dil; a.up = c.up;
  for (int i = 0; i < 8; ++i) a.off[i] = i < c.up ? c.off[i] : 0;
  a.la_in = c.la_in; a.lb_in = c.lb_in; a.la_out = c.la_out; a.lb_out = c.lb_out;
  a.mrf = c.mrf; a.mrf_div = c.mrf_div; a.slope = c.slope;
  const dim3 grid((c.nq + HG_TM - 1) / HG_TM, (c.cout + HG_TN - 1) / HG_TN, c.B * c.up);
  const double flops = 2.0 * c.B * c.up * (double)c.nq * c.cout * c.ntap * c.cin;
  const bool narrow = c.cout <= 32;
#define HG_GO(P, I, R) \
  s2st_launch("hifigan_conv<" #P "," #I "," #R ">", flops, 0.0, hifigan_conv_kernel<P, I, R>, grid, dim3(256), 0, st, a)
  if (c.precise) {
    if (narrow) HG_GO(true, true, 2);
    else HG_GO(true, true, 4);
  } else if (c.in_f32) {
    if (narrow) HG_GO(false, true, 2);
    else HG_GO(false, true, 4);
  } else {
    if (narrow) HG_GO(false, false, 2);
    else HG_GO(false, false, 4);
  }
#undef HG_GO
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}

int s2st_hifigan_post(const float* x, const float* w, const float* bias, float* wave, const int* frames, int la, int lb,
                      int B, int L, int C, int k, float slope, hipStream_t st) {
  if (C % 4 || k < 1) return S2ST_ERR_SHAPE;
  if (B <= 0 || L <= 0) return 0;
  const double flops = 2.0 * B * (double)L * C * k;
  s2st_launch("hifigan_post_kernel", flops, 0.0, hifigan_post_kernel, dim3((L + 255) / 256, B), dim3(256), 0, st, x, w, bias,
              wave, frames, la, lb, L, C, k, slope);
  return hipGetLastError() == hipSuccess ? 0 : S2ST_ERR_LAUNCH;
}
