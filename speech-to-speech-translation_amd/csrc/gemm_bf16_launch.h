// Host-side launch helpers shared by the bf16 GEMM forms (gemm_bf16.hip, gemm_bf16_w4.hip, gemm_bf16_p4.hip): the one
// operand-layout ladder and the one "configure once, launch with the instantiation's tag" step.
#pragma once
#include <type_traits>
#include "gemm_bf16_plan.h"
#include "s2st_ops.h"
#include "s2st_prof.h"

// as-launched work of one GEMM (profiling records): FLOPs, and the bytes it has to move at least -- both bf16
// operands once, the result once per output copy, the old value / residual once when it is read
struct GemmWork { double flops = 0, bytes = 0; };
inline GemmWork gemm_work(const GemmArgs& g) {
  const double mn = (double)g.M * g.N * g.batch;
  return GemmWork{2.0 * g.M * g.N * (double)g.K * g.batch,
                  2.0 * g.batch * ((double)g.M * g.K + (double)g.N * g.K) + mn * ((g.C.p ? 4 : 0) + (g.C.h ? 2 : 0)) +
                      mn * 4 * ((g.ep.accumulate ? 1 : 0) + (g.ep.resid ? 1 : 0))};
}
inline GemmWork gemm_work(const GemmGroup& grp) {
  GemmWork w;
  for (int i = 0; i < grp.n; ++i) { w.flops += gemm_work(grp.g[i]).flops; w.bytes += gemm_work(grp.g[i]).bytes; }
  return w;
}

// the empty problem of the preloads (M = N = K = 0: no loads, no stores) in operand layout `lay` (bit 0: A, bit 1: B K-contiguous)
inline GemmArgs empty_problem(int lay) {
  GemmArgs g{};
  g.A.dtype = g.B.dtype = S2ST_BF16;
  g.A.kmajor = lay & 1; g.B.kmajor = (lay >> 1) & 1;
  g.splitk = 1; g.zdiv = 1; g.tiles_n = 1; g.batch = 1; g.kchunk = GEMM_BK;
  return g;
}

// The operand layouts of arg (a GemmArgs, or a GemmGroup: its first problem's) as compile-time constants: calls
// f(A K-contiguous, B K-contiguous) with two std::bool_constant values.  ANY_A = false leaves the rows-contiguous A out
// (not instantiated: the 160-row tiles, whose padded A image exists K-contiguous only) and returns -1 for it.
inline const GemmArgs& first_problem(const GemmArgs& g) { return g; }
inline const GemmArgs& first_problem(const GemmGroup& grp) { return grp.g[0]; }
template <bool ANY_A = true, class ARG, class F>
int with_layouts(const ARG& arg, F&& f) {
  const bool akm = first_problem(arg).A.kmajor != 0, bkm = first_problem(arg).B.kmajor != 0;
  if (akm) return bkm ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  if constexpr (ANY_A) return bkm ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
  return -1;
}

// One launch of the instantiation (F, BM, BN, AKM, BKM, LAST) = kern: on its first use the dynamic-LDS limit is raised and
// its profiling tag is spelled (gemm_tag); the work figures are arg's
template <GemmForm F, int BM, int BN, bool AKM, bool BKM, bool LAST, class K, class ARG>
int launch_configured(K kern, int lds, dim3 grid, int threads, hipStream_t st, const ARG& arg) {
  static char tag[104];
  if (!tag[0]) {
    if (lds > 0 && hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return -1;
    gemm_tag(tag, sizeof tag, F, BM, BN, AKM, BKM, LAST);
  }
  const GemmWork w = gemm_work(arg);
  s2st_launch(tag, w.flops, w.bytes, kern, grid, dim3(threads), lds, st, arg);
  return 0;
}
