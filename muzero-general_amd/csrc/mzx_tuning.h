// mzx_tuning.h -- the library's tuning surface: ONE process-wide table of named integers behind the C ABI
// (include/mzx.h: mzx_tuning_set / mzx_tuning_get / mzx_tuning_name), instead of environment variables read inside
// launch paths.  Every entry is a routing or launch-shape choice that never changes WHAT is computed beyond the
// summation orders documented per entry; the defaults are the measured best, tests and bench.py
// move them for A/B runs.  Reads are plain loads (set a value before the calls it should affect, from the thread that
// makes them -- the same rule as for handles, mzx.h "Conventions").
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

namespace mzx {

struct TuningEntry {
  const char* name;
  int32_t value, dflt, lo, hi;
  const char* what;
};

enum TuningKey {
  TUNE_RB_HEADS = 0,          // head MLPs behind a tower's tail: 0 one launch per Linear layer, 2 one grouped launch per level
  TUNE_RB_TAIL,               // 1: scaling / small 1x1 head convolutions run inside the tower launch
  TUNE_RB_TOWER_T,            // > 0: samples per tower workgroup (0: the planner's cost model)
  TUNE_ROW_SPLIT_MIN,         // row-per-tree path: shards of at least this many trees run as two half-shards on two streams (0: never)
  TUNE_WIDE_TOWERS,           // 1: wide residual networks that also fit the LDS-resident engine search on the tower arithmetic (0: rz_search_kernel)
  TUNE_RT_SEARCH,             // tower whole-search kernel (rt_search_kernel): -1 automatic, 0 never, 1 whenever the network fits
  TUNE_RT_TREES,              // > 0: trees per workgroup of rt_search_kernel (0: the planner's cost model)
  TUNE_RT_WAVES,              // 4 / 8: waves per workgroup of rt_search_kernel (0: the planner's cost model)
  TUNE_RT_MAX_TREES,          // automatic routing: shards above this many trees stay on the two-stream streamed path
  TUNE_RT_DBG,                // timing experiments of rt_search_kernel (results are wrong with any bit set; never set in production)
  TUNE_RT_SHORT,              // 1: a last row group of MT - 1 row tiles runs the short K loop (0: every wave multiplies MT tiles, A/B)
  TUNE_ROUNDS_STREAMS,        // mzx_selfplay_rounds: 1 = every slot group behind the first searches on a stream of its own (0: one stream, A/B)
  TUNE_WAVE_SELECT,           // per-simulation launches, wide child records: 1 = a wavefront per tree walks (wave_select_kernel), 0 = a 16-lane row (row_select_kernel<0>, A/B); same walks
  TUNE_FCS_TM,                // streamed engine for fully connected networks: rows per workgroup, 16 / 32 / 64 (0: the rule fcs_choose_tm)
  TUNE_COUNT
};

inline TuningEntry* tuning_table() {
  static TuningEntry t[TUNE_COUNT] = {
      {"rb_heads", 2, 2, 0, 2, "head MLP levels: 0 = one launch per Linear layer, 2 = one grouped MFMA launch per level"},
      {"rb_tail", 1, 1, 0, 1, "tower tails (scaling, 1x1 head convolutions) inside the tower launch"},
      {"rb_tower_t", 0, 0, 0, 64, "samples per tower workgroup (0 = cost model)"},
      {"row_split_min", 1024, 1024, 0, 1 << 30, "two half-shards on two streams from this many trees (0 = never)"},
      {"wide_towers", 1, 1, 0, 1, "wide residual networks search on the tower arithmetic (0 = the LDS-resident whole-search kernel)"},
      {"rt_search", -1, -1, -1, 1, "tower whole-search kernel: -1 automatic, 0 never, 1 whenever supported"},
      {"rt_trees", 0, 0, 0, 16, "trees per workgroup of the tower whole-search kernel (0 = cost model)"},
      {"rt_waves", 0, 0, 0, 8, "waves per workgroup of the tower whole-search kernel: 4 or 8 (0 = cost model)"},
      {"rt_max_trees", 1 << 30, 1 << 30, 0, 1 << 30, "automatic routing: largest shard sent to the tower whole-search kernel"},
      {"rt_dbg", 0, 0, 0, 31, "timing experiments: 1 no K loops, 2 no epilogues, 4 no tree phases, 8 no staging / tails, 16 no head MLPs (wrong results)"},
      {"rt_short", 1, 1, 0, 1, "tower whole-search kernel: waves of a row group one tile short skip that tile's products (0 = multiply it, A/B)"},
      {"rounds_streams", 1, 1, 0, 1, "mzx_selfplay_rounds: slot groups behind the first search on streams of their own (0 = the caller's stream for all)"},
      {"wave_select", 1, 1, 0, 1, "per-simulation launches, more than 16 actions: the selection walk by a wavefront per tree (0 = a 16-lane row per tree, A/B; same walks)"},
      {"fcs_tm", 0, 0, 0, 64, "streamed engine for fully connected networks: rows per workgroup, the largest of 16 / 32 / 64 that fits LDS and is not above the value, values below 16 count as 16 (0 = the largest that fits and leaves a workgroup per compute unit; same bits)"},
  };
  return t;
}

inline int32_t tune(TuningKey k) { return tuning_table()[k].value; }

// Latency / layout EXPERIMENTS of earlier rounds (knock-outs, forced tilings, phase stamps; profiles/r0*_experiments*.txt)
// are environment variables -- in instrumented builds only (MZX_CXXFLAGS=-DMZX_EXPERIMENT, muzero-general_amd/build.py).  The
// product library never reads the environment: every such knob is its default there.
inline int exp_int(const char* name, int dflt) {
#ifdef MZX_EXPERIMENT
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
#else
  (void)name;
  return dflt;
#endif
}

// Which GEMMs of a residual training step take the LDS-tiled body (mzx_train_gemm_tiled.h) instead of the wave body, under
// the handle's switch (mzx_net_set_train_gemm: 0 none, 1 this rule, 2 all).  Both bodies return the same bits, so the rule
// is a pure tuning decision: a 64 x 64 workgroup tile needs rows and columns to fill it, and enough workgroups
// (tiles x weight-gradient chunks) to occupy the device's 256 compute units -- below that the wave body's four times as many,
// smaller work items spread better.
constexpr int TRAIN_GEMM_TILED_MIN_M = 64;
constexpr int TRAIN_GEMM_TILED_MIN_N = 32;
constexpr int TRAIN_GEMM_TILED_MIN_WORKGROUPS = 256;
inline bool train_gemm_tiled(int mode, int64_t M, int64_t N, int64_t chunks) {
  if (mode != 1) return mode == 2;
  return M >= TRAIN_GEMM_TILED_MIN_M && N >= TRAIN_GEMM_TILED_MIN_N &&
         ((M + 63) / 64) * ((N + 63) / 64) * chunks >= TRAIN_GEMM_TILED_MIN_WORKGROUPS;
}

// Which of the GEMMs the rule above leaves on the wave body take the in-workgroup split-K body (mzx_train_gemm_ksplit.h)
// instead, under the handle's switch (3 this rule, 4 all, any other mode none).  The body cuts the dependent chain over K into
// four, one per wave of a 32 x 32 workgroup tile, so a GEMM needs at least four k-groups of 16 per weight-gradient chunk --
// below that a wave idles and the LDS join is pure overhead.  `chunks` chunks of RTN_KCHUNK = 512 positions: with more than
// one, every chunk but the last is 512 long.  The rows and columns asked for started at one full 32 x 32 tile and were lowered
// to one full MFMA tile each way by the first measurement (profiles/resnet_train_ksplit_bench_rule32.log): at 16
// channels that rule picked 0 of 164 GEMMs at tic-tac-toe 64 x 21 and 0 of 159 at breakout 16 x 6, where sending EVERY GEMM to
// the body took the step from 4.98 to 4.11 ms and from 9.96 to 8.85 ms (spreads below 0.06 ms): the body pays off with half of
// its tile empty.  The heads' GEMMs of a few reduced channels stay on the wave body.
constexpr int TRAIN_GEMM_KSPLIT_MIN_M = 16;
constexpr int TRAIN_GEMM_KSPLIT_MIN_N = 16;
constexpr int TRAIN_GEMM_KSPLIT_MIN_K = 64;
inline bool train_gemm_ksplit(int mode, int64_t M, int64_t N, int64_t K, int64_t chunks) {
  if (mode != 3) return mode == 4;
  return M >= TRAIN_GEMM_KSPLIT_MIN_M && N >= TRAIN_GEMM_KSPLIT_MIN_N && (chunks > 1 || K >= TRAIN_GEMM_KSPLIT_MIN_K);
}

// Rows per workgroup (TM = 16, 32 or 64) of the streamed engine for fully connected networks (mzx_fc_streamed.h).  fits[i]: the
// LDS plan of TM = 16 << i fits.  The largest TM that fits and still gives every compute unit a workgroup -- 256 of them, the
// MI355X's count, a constant as TRAIN_GEMM_TILED_MIN_WORKGROUPS above -- else the smallest that fits: below 256 workgroups
// more, smaller tiles spread better.  forced (the tuning entry "fcs_tm", tests): the largest TM that fits and is not above
// it; a value below 16 counts as 16.  A row's bits do not depend on TM, so this is a pure tuning decision.  0: nothing fits.
constexpr int FCS_MIN_WORKGROUPS = 256;
inline int fcs_tm_rule(int batch, int forced, const bool fits[3]) {
  if (forced > 0 && forced < 16) forced = 16;
  int smallest = 0;
  for (int i = 2; i >= 0; --i) {
    const int TM = 16 << i;
    if (!fits[i] || (forced > 0 && TM > forced)) continue;
    if (forced > 0 || (batch + TM - 1) / TM >= FCS_MIN_WORKGROUPS) return TM;
    smallest = TM;
  }
  return smallest;
}

inline int tuning_find(const char* name) {
  if (!name) return -1;
  TuningEntry* t = tuning_table();
  for (int i = 0; i < TUNE_COUNT; ++i)
    if (strcmp(t[i].name, name) == 0) return i;
  return -1;
}

}  // namespace mzx
