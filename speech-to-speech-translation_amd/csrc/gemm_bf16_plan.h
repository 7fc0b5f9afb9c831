// What the bf16 GEMM launcher (gemm_bf16.hip) decides, as pure host code: which kernel form runs a product, on which tile,
// with which split of K, which epilogue marks and which grid.  No HIP call, no environment read, no statics: the switches
// (GemmSwitches) and the chip (GemmChip) are arguments, pointers are looked at for null and alignment only -- so the whole
// decision can be read top to bottom here, and tested for a 256-CU chip on a machine without one (s2st_gemm_plan_f32,
// tests/test_gemm_dispatch.py).  s2st_gemm_bf16 / s2st_gemm_bf16_group are: fill the switches, plan, launch the plan's form.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "s2st_hip.h"

typedef s2st_gemm_operand GemmOperand;
typedef s2st_gemm_args GemmArgs;

constexpr int GEMM_BK = 64;  // K-step of every bf16 form
#define S2ST_GROUP_MAX 8
#define S2ST_STREAMK_MAX_WGS 512
#define S2ST_STREAMK_SCRATCH_FLOATS (1024 + (long)S2ST_STREAMK_MAX_WGS * 128 * 128)

// Every environment switch the dispatcher reads, with its default.  Filled by gemm_switches() in
// gemm_bf16.hip: dma, splitk_target and persist_wgs once per process, the others per call (A/B switches the tests flip).
struct GemmSwitches {
  int dma = 1;              // S2ST_GEMM_DMA=0: the register-staged kernel everywhere (no LDS-DMA ring) -- the A/B switch of round 1
  bool tile_set = false;    // S2ST_GEMM_TILE=<bm>x<bn> (tuning aid) forces the tile; an unparsable value means 64 x 64
  int tile_bm = 64, tile_bn = 64;
  // S2ST_GEMM_W4: 0 = the 8-wave ring kernels only (one workgroup per CU); -1 (default) = the 4-wave early-release form
  // (gemm_bf16_w4.hip, 2 - 3 workgroups per CU) for single products with at least one 128 x 128 tile per CU, see w4_pick();
  // 1 = every 128-row single product on it; 2 = grouped weight gradients too
  int w4 = -1;
  // S2ST_GEMM_P4: 0 = never; -1 (default) = the 256 x 256 four-phase form (gemm_bf16_p4.hip) where p4_pick() says so; 1 = every
  // product it can run
  int p4 = -1;
  // S2ST_GEMM_PERSIST: 0 = one-shot kernels only, 1 = grouped launches persistent, single products one-shot (default:
  // with more tiles than CUs the hardware dispatcher back-fills CUs as one-shot workgroups retire, which balances better
  // than a fixed walk of 2.25 tiles per workgroup -- 10.05 vs 10.58 ms per training step, profiles/r02_ab_switches.txt),
  // 2 = every 128-row launch persistent, 3 = grouped launches and single products with more tiles than CUs
  // (gemm_switches() holds it to 0 / 1 in builds without the persistent kernels, and streamk to 0)
  int persist = 1;
  int persist_wgs = 0;      // S2ST_GEMM_PERSIST_WGS=<n> (tuning aid): the CU count the pickers and the persistent grids use
  // S2ST_GEMM_STREAMK: 0 = whole tiles per workgroup, 1 = stream-K where a scratch buffer is bound to the stream.  On by
  // default for callers that bind a scratch themselves (s2st_gemm_streamk_scratch); the training engine binds one only
  // with S2ST_GEMM_STREAMK=1 in the environment: measured on MI355X (tools/streamk_probe.py) the
  // hand-off -- L2 write-back behind the release, invalidate + 64 KB read behind the acquire -- costs 12-20 us per launch,
  // more than the idle last round of the 25-45 us products of a training step; it pays from ~2 rounds of long-K tiles on.
  int streamk = 1;
  int streamk_min_steps = 8;  // S2ST_STREAMK_MIN_STEPS
  bool fast_epi = true;       // S2ST_GEMM_FAST_EPI=0: the general epilogue everywhere (A/B switch)
  int splitk_target = 128;    // S2ST_SPLITK_TARGET: workgroups a split-K launch aims for
  // S2ST_GROUP_TILE=256: 256 x 128 tiles (48 KB of operands per K-step for twice the FLOPs: half the workgroups, which
  // leaves CUs to the data-path stream the group runs beside)
  int group_tile = 0;
  // default: one workgroup per tile of the concatenated list (plain K-loop: 9.65 vs 9.76 ms/step);
  // S2ST_GROUP_ONESHOT=0: the persistent tile walk (also what S2ST_GROUP_TILE=256 and a bound stream-K scratch use)
  bool group_oneshot = true;
};

// experimental: a -DS2ST_EXPERIMENTAL build, the only one that carries the persistent walk, stream-K and the 256 x 128 tile
struct GemmChip { int ncu; int slots160; bool experimental; };

enum GemmForm {
  GEMM_STAGED, GEMM_RING, GEMM_W4, GEMM_P4, GEMM_PERSISTENT, GEMM_RING_256x128,
  GEMM_GROUP_RING, GEMM_GROUP_W4, GEMM_GROUP_PERSISTENT, GEMM_GROUP_PERSISTENT_256
};

struct GemmPlan {
  int error = 0;  // S2ST_ERR_*: nothing is launched
  GemmForm form = GEMM_STAGED;
  int bm = 0, bn = 0, splitk = 1, kchunk = 0, tiles_n = 0, vec = 0, cvec = 0, grid_x = 0, grid_y = 1;
  bool use_slab = false;
  bool akm = false, bkm = false;
  bool sk = false;  // persistent forms: the stream-K walk (needs the scratch bound to the stream)
  // persistent and grouped forms: the concatenated tile list; cvec_of[i] = problem i's epilogue marks
  int n = 0, total = 0, tile0[S2ST_GROUP_MAX + 1] = {0}, cvec_of[S2ST_GROUP_MAX] = {0};
};

// ---- the instantiation behind a (form, tile): ring stages, waves, interleaved steady state --------------------------------
// (one instantiation per tile shape: the interleaved steady state, 8 waves for 128-row tiles; the round-2 A/B forms
// -- plain loop, 4 waves, 2 / 3 / 5 ring stages, 64 x 128 -- were measured then and are no longer built)
constexpr int ring_ns(int bm) { return bm == 256 ? 3 : 4; }
constexpr int ring_nw(int bm) { return bm == 64 ? 4 : 8; }
constexpr bool ring_il(int bm) { return bm != 256; }
// two ring slots: 128 x 64 is 48 KB, three workgroups per CU (what w4_pick's slot count assumes; 4584 x 2048 x 512: 18.3 us against
// 22.0 us with three slots = two workgroups per CU, measured in round 3)
constexpr int W4_NS = 2;

// profiling tag of an instantiation, spelled like the kernel name in a rocprofv3 kernel trace.  last: VEC of the staged
// kernels, stream-K of the persistent ones
inline void gemm_tag(char* buf, size_t cap, GemmForm f, int bm, int bn, bool akm, bool bkm, bool last) {
  const char *a = akm ? "true" : "false", *b = bkm ? "true" : "false", *l = last ? "true" : "false";
  switch (f) {
    case GEMM_STAGED: snprintf(buf, cap, "gemm_bf16_kernel<%d, %d, %s, %s, %s>", bm, bn, a, b, l); break;
    case GEMM_RING: case GEMM_RING_256x128: case GEMM_GROUP_RING:
      snprintf(buf, cap, "gemm_bf16_dma%s_kernel<%d, %d, %s, %s, %d, %d, %s>", f == GEMM_GROUP_RING ? "_group" : "", bm, bn, a, b,
               ring_ns(bm), ring_nw(bm), ring_il(bm) ? "true" : "false");
      break;
    case GEMM_W4: case GEMM_GROUP_W4:
      snprintf(buf, cap, "gemm_bf16_w4%s_kernel<%d, %d, %s, %s, %d>", f == GEMM_GROUP_W4 ? "_group" : "", bm, bn, a, b, W4_NS);
      break;
    case GEMM_P4: snprintf(buf, cap, "gemm_bf16_p4_kernel<256, 256>"); break;
    default:
      snprintf(buf, cap, "gemm_bf16_dma_persistent_kernel<%d, %d, %s, %s, %d, %d, %s>", bm, bn, a, b, ring_ns(bm), ring_nw(bm), l);
  }
}

// ---- predicates ------------------------------------------------------------------------------------------------------------
inline long gemm_tiles(const GemmArgs& g, int bm, int bn) { return (long)((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * g.batch; }

// 16-byte fast path: aligned base, ld and batch strides multiples of 8 elements.  (K tails are
// masked in the kernel; rows-contiguous operands rely on the padded-row contract.)
inline bool vec_ok(const GemmOperand& o) {
  return ((uintptr_t)o.p % 16 == 0) && (o.sp.ld % 8 == 0) && (o.sp.bs % 8 == 0) && (o.zo % 8 == 0) && (o.zi % 8 == 0);
}

// LDS-DMA ring kernels: rows-contiguous operands need a plain k stride
inline bool dma_layout_ok(const GemmArgs& g) { return (g.A.kmajor || g.A.sp.per <= 0) && (g.B.kmajor || g.B.sp.per <= 0); }

// alignment flags the kernels / epilogue read: whether the 16-byte operand path applies (avec = bvec), and bit 0 of cvec
inline bool prep_flags(const GemmArgs& g, int* cvec) {
  *cvec = ((!g.C.p || (uintptr_t)g.C.p % 16 == 0) && (!g.C.h || (uintptr_t)g.C.h % 8 == 0) &&
           g.C.sp.ld % 4 == 0 && g.C.sp.bs % 4 == 0 && g.C.zo % 4 == 0 && g.C.zi % 4 == 0 &&
           (!g.ep.resid || (uintptr_t)g.ep.resid % 16 == 0) && (!g.ep.bias || ((uintptr_t)g.ep.bias % 16 == 0 && g.ep.bias_zo % 4 == 0)))
              ? 1 : 0;
  return vec_ok(g.A) && vec_ok(g.B);
}

// bit 1 of cvec: the straight-line epilogue applies (gemm_epilogue_fast; S2ST_GEMM_FAST_EPI=0 is the A/B switch).
// Takes the split-K / slab decisions already made; returns cvec with bits 1 .. 3 set.
inline int mark_fast_epilogue(const GemmArgs& g, int cvec, bool unsplit, const GemmSwitches& sw) {
  cvec &= 1;
  if (!sw.fast_epi) return cvec;
  const bool drop = g.ep.drop_p > 0.f, res = g.ep.resid != nullptr, accu = g.ep.accumulate != 0;
  const bool combo = !accu || (!drop && !res && !g.C.h);  // instantiated: {-, resid, drop, drop + resid} x outputs, accumulate (fp32)
  // the bf16 copy is stored 16 bytes (8 columns) per lane
  const bool h16 = !g.C.h || ((uintptr_t)g.C.h % 16 == 0 && g.C.sp.ld % 8 == 0 && g.C.sp.bs % 8 == 0 && g.C.zo % 8 == 0 &&
                              g.C.zi % 8 == 0 && g.N % 8 == 0);
  if (cvec && g.N >= 4 && g.N % 4 == 0 && g.M >= 1 && unsplit && !g.ep.mask_y && !g.ep.colsum && !g.ep.colsum_part &&
      (g.ep.act != 2 || (!drop && !accu)) && combo && h16 && (g.C.p || g.C.h) && (!accu || g.C.p))
    cvec |= 2;
  // bit 3: the masked data-gradient form (bf16 output only, nothing else in the epilogue but the column sums)
  if (cvec && g.ep.mask_y && g.C.h && !g.C.p && h16 && g.N >= 8 && g.M >= 1 && unsplit && !g.ep.bias &&
      g.ep.act == 0 && !drop && !res && !accu && (uintptr_t)g.ep.mask_y % 16 == 0)
    cvec |= 8;
  return cvec;
}

// Which form runs a single product (measured per shape on MI355X with tools/gemm_forms_bench.py, kernel time from
// events attached to the dispatch, profiles/r03_gemm_forms.txt).  With fewer 128 x 128 tiles than CUs (M ~ 4.6 k tokens x
// N = 512: 144 tiles) nothing co-resides anyway and the 8-wave kernel's faster K-loop wins (17.5 vs 23.9 us at K = 2048);
// from one tile per CU on, two or three co-resident workgroups hide each other's prologue / epilogue / barrier waits:
// N = 1536 ... 2048 at K = 512 run 10 - 30 % shorter (4584 x 2048 x 512: 17.5 vs 21.4 us; 2800 x 1536 x 512: 11.1 vs 15.8).
// Between the two 4-wave shapes the fuller last round wins: 128 x 128 tiles over 2 slots per CU against 128 x 64 tiles
// over 3 (the pick agreed with the faster of the two on every measured shape).
// Round 8, 160 x 128 tiles (K-contiguous A): the same rounds-of-slots count.  Where the 128-row pick needs a second round
// and 160-row tiles fit the chip's slots in ONE (N = 2048 with 4096 < M <= 5120: 33 - 40 row tiles x 16 against 512 slots,
// <= 32 x 16 with 160 rows), one round of 1.25x tiles beats 1.1 - 1.25 rounds: 23.0 -> 17.7 us was the step at M = 4096
// (profiles/r06_gemm_m_sweep.txt; tools/gemm_m_sweep.py now runs to M = 5120).  With one
// round either way (M <= 4096; N = 1536) the smaller tile stays, and products of many rounds are not touched.
// Returns 0 (8-wave kernels), else bn of the 4-wave form; *bm gets its tile rows (128 or 160).
inline bool tile160_ok(const GemmArgs& g) { return g.A.kmajor && g.A.sp.per <= 0 && g.batch == 1; }

inline int w4_pick(const GemmArgs& g, const GemmSwitches& sw, const GemmChip& chip, int* bm) {
  *bm = 128;
  if (sw.w4 == 0 || g.M < 128) return 0;
  const long t128 = gemm_tiles(g, 128, 128), t64 = gemm_tiles(g, 128, 64);
  if (sw.w4 < 0 && t128 < chip.ncu) return 0;
  const long s128 = 2L * chip.ncu, s64 = 3L * chip.ncu;
  const double e128 = (double)t128 / (double)(((t128 + s128 - 1) / s128) * s128);
  const double e64 = (double)t64 / (double)(((t64 + s64 - 1) / s64) * s64);
  if (tile160_ok(g) && g.N > 64) {
    const long t160 = gemm_tiles(g, 160, 128);
    const long s160 = (long)chip.slots160 * chip.ncu;
    if (t160 <= s160 && t128 > s128 && t64 > s64) { *bm = 160; return 128; }
  }
  // Round 5: many rounds of long K-loops are priced by the steady state, not by the last round's fill -- per flop the
  // 128 x 128 tile needs 2/3 of the LDS reads of the 128 x 64 one.  HuBERT's conv stack (307 k / 154 k rows x 512 x 1536):
  // 632 vs 750 us and 342 vs 402 us, where the fill rule took 128 x 64 (25.0 full rounds against 18.75);
  // tools/conv_forms_bench.py, profiles/r05_hubert_forms.txt.  (The training step's products have < 4 rounds: unchanged.)
  if (g.N > 64 && g.K >= 1024 && t128 >= 4 * s128) return 128;
  return (g.N > 64 && e128 >= e64) ? 128 : 64;
}

// The four-phase form can run: both operands K-contiguous with plain row strides, 16-byte aligned (the caller checked: the
// LDS-DMA kernels apply), batch 1, no split-K, no masked epilogue.  The pick is a two-line cost model fitted to
// tools/gemm_p4_bench.py (profiles/r05_gemm_p4_bench.txt, random operands, kernel time from events on the dispatch):
//   four-phase form : rounds of 256-row tiles over the CUs x (2.0 us per 64-deep K-tile + 7 us of prologue / epilogue)
//   128-row forms   : ~650 TFLOP/s on products of this size (577 - 693 measured; 870 on 4096^3)
// It takes 4096^3 (126 vs 159 us: 1.09 PFLOP/s), HuBERT's FFN-in products (9600 x 3072 x 768: 64 vs 78 us; 19200 rows: 119 vs
// 148) and leaves the K = 512 products of the training step (one round of 8 K-tiles: 21 vs 14 - 19 us) and the short-N
// ones (768 columns: a third of the CUs) where they were.
inline bool p4_can(const GemmArgs& g) {
  return g.A.kmajor && g.B.kmajor && g.batch == 1 && g.A.sp.per <= 0 && g.B.sp.per <= 0 && !g.ep.mask_y &&
         !g.ep.colsum && !g.ep.colsum_part;
}
inline bool p4_pick(const GemmArgs& g, const GemmSwitches& sw, const GemmChip& chip) {
  if (sw.p4 >= 1) return true;
  if (g.M < 512 || g.N < 512 || g.K < 8 * GEMM_BK) return false;
  const long ncu = chip.ncu;
  const long rounds = (gemm_tiles(g, 256, 256) + ncu - 1) / ncu;
  const double t_p4 = (double)rounds * (2.0 * ((g.K + GEMM_BK - 1) / GEMM_BK) + 7.0);  // us
  const double t_ring = 2.0 * g.M * (double)g.N * g.K / 650e6;                          // us at 650 TFLOP/s
  // (0.80, not parity: beside a training step -- HuBERT's front end runs ahead on a second stream -- a 512-thread workgroup
  // holding 128 KB of LDS for tens of microseconds keeps the step's short dependent kernels off its CU; with the threshold
  // at 0.92 the front end's FFN-in products took this form, 64 vs 78 us alone, and config 3 / 4 got SLOWER: 10.77 - 11.0
  // vs 10.63 ms per step, profiles/r05_hubert_p4_ab.txt)
  return t_p4 < 0.80 * t_ring;
}

// Stream-K for a persistent launch of `total` 128 x 128 tiles with `steps` K-steps in all: when the split pays -- uneven
// rounds of whole tiles (or fewer tiles than CUs) and enough K-steps per workgroup that the partial-sum hand-off (64 KB
// out, 64 KB in) is small change
inline bool streamk_pays(long total, long steps, const GemmSwitches& sw, const GemmChip& chip) {
  const int G = chip.ncu & ~7;
  if (sw.streamk <= 0 || total <= 0 || G < 8 || G > S2ST_STREAMK_MAX_WGS) return false;
  const long rounds = (total + G - 1) / G;
  const double waste = 1.0 - (double)total / (double)(rounds * G);  // idle share of the last round
  return waste > 0.08 && steps >= (long)sw.streamk_min_steps * G;
}

// grid of a persistent launch: one workgroup per CU at most (stream-K: per CU of whole XCDs); (preload: no tiles)
inline int persistent_grid(int total, bool sk, const GemmChip& chip) {
  return sk ? (chip.ncu & ~7) : (total < 1 ? 1 : (total < chip.ncu ? total : chip.ncu));
}

// ---- one product ------------------------------------------------------------------------------------------------------------
// sk_bound: a stream-K scratch is bound to the launch's stream.  g.zdiv is not looked at.
inline GemmPlan plan_single(const GemmArgs& g, const GemmSwitches& sw, const GemmChip& chip, bool sk_bound) {
  GemmPlan p;
  auto fail = [&](int code) { p.error = code; return p; };
  p.akm = g.A.kmajor != 0;
  p.bkm = g.B.kmajor != 0;
  int cvec0;
  const bool vec = prep_flags(g, &cvec0);
  p.vec = vec ? 1 : 0;
  if (g.ep.mask_y && (!cvec0 || g.N % 4 != 0)) return fail(S2ST_ERR_SHAPE);
  const bool dma_ok = vec && sw.dma && dma_layout_ok(g);  // the LDS-DMA kernels: aligned operands, plain k strides
  const bool can160 = dma_ok && tile160_ok(g) && sw.persist <= 1;
  const bool linear_epi = !g.ep.act && g.ep.drop_p == 0.f && !g.ep.mask_y;
  const bool may_split = g.ep.accumulate && linear_epi && g.C.p && !g.C.h && !g.ep.bias && !g.ep.resid && g.K >= 8 * GEMM_BK;
  const int kt = (g.K + GEMM_BK - 1) / GEMM_BK;
  int bm = 64, bn = 64;

  // 1. cost pick: estimated time = rounds over the CUs x per-tile work / per-tile efficiency
  // (tile-preference weights: round 2's sweep.  160 x 64, round 8: the 128 x 64 kernel with five row blocks per wave, so
  //  its weight -- a candidate only where it runs in ONE round, K-contiguous A, on the LDS-DMA kernels: N = 512 with
  //  4096 < M <= 5120, where 128 x 64 needs a second round and the pick used to fall to 144 - 160 tiles of 128 x 128)
  if (vec) {
    const struct { int bm, bn; double eff; } cands[4] = {{128, 128, 1.0}, {128, 64, 0.8}, {160, 64, 0.8}, {64, 64, 0.55}};
    double best = 1e300;
    for (const auto& c : cands) {
      const long tiles = gemm_tiles(g, c.bm, c.bn), rounds = (tiles + chip.ncu - 1) / chip.ncu;
      if (c.bm == 160 && !(can160 && rounds == 1 && (!may_split || tiles >= sw.splitk_target))) continue;  // (never a product that would split K)
      // split-K candidates fill the chip anyway: cost by work / efficiency only
      const double cost = (double)rounds * c.bm * c.bn / c.eff;
      if (cost < best) { best = cost; bm = c.bm; bn = c.bn; }
    }
  }

  // 2. forced tile (vector path only).  160x128 (4-wave form) / 160x64 (8-wave ring form): where the product cannot take
  // them, the 128-row tile of that width.  256x256: the four-phase form where it can run (step 5).  256x128: the ring
  // kernel of experimental builds; elsewhere 128 x 128
  const bool forced = vec && sw.tile_set;
  if (forced) {
    bm = sw.tile_bm;
    bn = sw.tile_bn;
    if (bm == 160 && !(can160 && (bn == 128 || bn == 64))) bm = 128;
  }
  const bool forced_p4 = forced && bm == 256 && bn == 256;
  if (bm == 256 && !forced_p4 && !(chip.experimental && dma_ok && g.batch == 1)) { bm = 128; bn = 128; }

  // 3. split-K eligibility: only accumulating fp32 outputs with a linear epilogue (weight gradients); a 160-row tile, picked
  // or forced, runs K unsplit.  A product that will split (fewer than 256 tiles of 128 x 128) takes that tile and no other form
  const bool can_split = may_split && bm != 160;
  const bool split_like = can_split && gemm_tiles(g, 128, 128) < 256;
  if (vec && split_like) { bm = 128; bn = 128; }
  const bool other_forms = dma_ok && !split_like && sw.persist != 2;

  // 4. the 4-wave early-release form: a forced tile is honoured (S2ST_GEMM_W4 >= 1 puts it on that form)
  bool w4 = false;
  if (other_forms) {
    int w4bm = 128, w4bn;
    if (!forced) w4bn = w4_pick(g, sw, chip, &w4bm);
    else if (bm == 160 && bn == 128) { w4bn = 128; w4bm = 160; }  // (the 4-wave form is the only 160 x 128 one)
    else w4bn = (sw.w4 >= 1 && bm == 128 && (bn == 128 || bn == 64)) ? bn : 0;
    if (w4bn) { w4 = true; bm = w4bm; bn = w4bn; }
  }

  // 5. the 256 x 256 four-phase form; a forced tile is honoured where the form can run at all
  const bool p4_takes = other_forms && p4_can(g) && sw.p4 != 0 && (forced ? forced_p4 : p4_pick(g, sw, chip));
  // (the four-phase kernel has no split-K form, so a product that then splits K -- fewer than 256 tiles of
  //  256 x 256 -- goes back to 128 x 128 tiles BEFORE the grid is derived.)
  const bool p4 = p4_takes && !(can_split && gemm_tiles(g, 256, 256) < 256);
  if (p4_takes) w4 = false;
  if (p4) { bm = 256; bn = 256; }
  else if (p4_takes || forced_p4) { bm = 128; bn = 128; }

  // 6. split-K geometry: K is split over workgroups; partial sums go to fp32 slabs in the caller's scratch and are combined
  // by splitk_reduce_kernel (HBM/MALL streaming, ~5 TB/s), or -- without scratch -- are added
  // with fp32 atomics (~1.3 TB/s chip-wide, so only a fallback).
  const int tm = (g.M + bm - 1) / bm, tn = (g.N + bn - 1) / bn;
  const long nt = (long)tm * tn * g.batch;
  int splitk = 1;
  if (can_split && nt < 256) {
    const int want = (int)((sw.splitk_target + nt - 1) / nt), maxs = g.K / (4 * GEMM_BK);
    splitk = want < maxs ? want : maxs;
    if (g.ws) {
      const long fit = g.ws_floats / ((long)g.M * g.N * g.batch);
      if (fit < splitk) splitk = (int)fit;
    }
    if (splitk < 1) splitk = 1;
  }
  p.kchunk = ((kt + splitk - 1) / splitk) * GEMM_BK;
  splitk = (g.K + p.kchunk - 1) / p.kchunk;
  p.splitk = splitk < 1 ? 1 : splitk;
  p.use_slab = p.splitk > 1 && g.ws != nullptr;
  p.cvec = mark_fast_epilogue(g, cvec0, p.splitk == 1 && !p.use_slab, sw);
  p.bm = bm;
  p.bn = bn;
  p.tiles_n = tn;
  p.grid_x = tm * tn;
  p.grid_y = g.batch * p.splitk;
  if (p.grid_y > 65535) return fail(S2ST_ERR_SHAPE);
  const bool unsplit = p.splitk == 1;

  // 7. persistent / stream-K eligibility (experimental builds): more tiles than CUs -- the persistent kernel keeps the DMA
  // ring running across the tiles a workgroup walks -- and, with a stream-K scratch bound to the stream, also the 128 x 128
  // launches that leave CUs idle (N = 512 layers: 144 tiles) when K is long enough to share (streamk_pays decides)
  const bool sk_form = sk_bound && sw.streamk > 0 && bm == 128 && bn == 128;
  if (dma_ok && g.batch == 1 && unsplit && bm == 128 && (bn == 128 || bn == 64) && sw.persist > 0 && !w4 &&
      (sw.persist == 2 || (sw.persist == 3 && nt > chip.ncu) || (sk_form && (nt > chip.ncu || nt * kt >= 8L * chip.ncu)))) {
    if (!chip.experimental) return fail(S2ST_ERR_ARG);  // (not built; gemm_switches() never lets a product build get here)
    p.form = GEMM_PERSISTENT;
    p.n = 1;
    p.total = p.tile0[1] = (int)nt;
    p.cvec_of[0] = p.cvec;
    p.sk = sk_form && streamk_pays(nt, nt * kt, sw, chip);
    p.grid_x = persistent_grid(p.total, p.sk, chip);
    return p;
  }

  // the form; a tile none of its kernels is built for (a forced one) is an error, not a launch on another tile's grid
  const bool t128 = bm == 128 && (bn == 128 || bn == 64), t64 = bm == 64 && bn == 64;
  if (!dma_ok) p.form = GEMM_STAGED;
  else if (p4 && unsplit) p.form = GEMM_P4;
  else if (w4 && unsplit) p.form = GEMM_W4;
  else if (bm == 256 && bn == 128) p.form = GEMM_RING_256x128;
  else p.form = GEMM_RING;
  const bool built = p.form == GEMM_P4 || p.form == GEMM_RING_256x128 || t128 || t64 ||
                     (bm == 160 && (p.form == GEMM_W4 ? bn == 128 : p.form == GEMM_RING && bn == 64));
  if (!built) return fail(S2ST_ERR_ARG);
  return p;
}

// ---- a group ------------------------------------------------------------------------------------------------------------------
// true if g can join a group (aligned bf16 operands, plain strides, batch 1, >= 128 x 128 of output)
inline bool group_member_ok(const GemmArgs& g, const GemmSwitches& sw) {
  if (g.A.dtype != S2ST_BF16 || g.B.dtype != S2ST_BF16 || g.precise || sw.persist == 0) return false;
  int cvec;
  if (!sw.dma || !prep_flags(g, &cvec) || !dma_layout_ok(g) || g.batch != 1 || g.M < 128 || g.N < 128 || g.K < 1) return false;
  return !(g.ep.mask_y && (!cvec || g.N % 4 != 0));
}

// list[0..n): problems that passed group_member_ok, all with the layouts of list[0]; every one runs K unsplit
inline GemmPlan plan_group(const GemmArgs* list, int n, const GemmSwitches& sw, const GemmChip& chip, bool sk_bound) {
  GemmPlan p;
  p.form = GEMM_GROUP_RING;
  if (n <= 0) return p;
  if (n > S2ST_GROUP_MAX) { p.error = S2ST_ERR_ARG; return p; }
  p.akm = list[0].A.kmajor != 0;
  p.bkm = list[0].B.kmajor != 0;
  p.vec = 1;
  bool big = chip.experimental && sw.group_tile == 256;
  for (int i = 0; i < n; ++i) big = big && list[i].M >= 256;
  p.bm = big ? 256 : 128;
  p.bn = 128;
  long steps = 0;
  for (int i = 0; i < n; ++i) {
    const GemmArgs& g = list[i];
    int cvec;
    if (!prep_flags(g, &cvec) || g.A.kmajor != list[0].A.kmajor || g.B.kmajor != list[0].B.kmajor) { p.error = S2ST_ERR_ARG; return p; }
    p.cvec_of[i] = mark_fast_epilogue(g, cvec, true, sw);
    const int tiles = (int)gemm_tiles(g, p.bm, p.bn);
    p.tile0[i + 1] = p.tile0[i] + tiles;
    steps += (long)tiles * ((g.K + GEMM_BK - 1) / GEMM_BK);
  }
  p.n = n;
  p.total = p.tile0[n];
  p.cvec = p.cvec_of[0];
  p.tiles_n = (list[0].N + p.bn - 1) / p.bn;
  p.kchunk = ((list[0].K + GEMM_BK - 1) / GEMM_BK) * GEMM_BK;
  if (big) p.form = GEMM_GROUP_PERSISTENT_256;
  else if (!chip.experimental || (sw.group_oneshot && !(sk_bound && sw.streamk > 0)))
    p.form = sw.w4 >= 2 ? GEMM_GROUP_W4 : GEMM_GROUP_RING;
  else p.form = GEMM_GROUP_PERSISTENT;
  if (p.form == GEMM_GROUP_RING || p.form == GEMM_GROUP_W4) { p.grid_x = p.total < 1 ? 1 : p.total; return p; }
  p.sk = sk_bound && p.form == GEMM_GROUP_PERSISTENT && streamk_pays(p.total, steps, sw, chip);
  p.grid_x = persistent_grid(p.total, p.sk, chip);
  return p;
}
