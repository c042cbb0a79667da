// mzx_replay.h -- hand-off of finished games to the replay buffer: the INITIAL prioritised-replay priorities of a
// shard's games on the device, and the device-resident replay store (second half of the file):
// n-step values of ragged games, make_target for a training batch, and the reanalyse sweep (the positions of ragged games
// as a sample list, the decoded values of a chunk written into the pool).
//
// Reference: ReplayBuffer.save_game, /root/reference/replay_buffer.py:39-51 -- for every position i of a game
//     priority_i = |root_value_i - compute_target_value(game, i)| ** PER_alpha        (numpy.float64, then float32)
//     game_priority = max_i priority_i
// with compute_target_value (:230-262): the root value td_steps ahead (sign by whose turn it is there) times
// discount ** td_steps -- or the integer 0 past the end of the game --, plus the rewards of the next td_steps moves, each
// signed by whose turn it was and times discount ** i, accumulated in that order in binary64.
//
// One element per (game, position); G games of T positions each (a shard record: games that started and ended together;
// ragged shards go record by record).  Bit-exactness: the target value and the gap |root - target| use only binary64
// multiplications and additions in the reference's order (the library is compiled with -ffp-contract=off), with
// discount ** i taken from a table the HOST fills with Python's own float pow -- identical bit patterns to the reference
// (`d_targets` exposes them to the tests).  The final `** PER_alpha` is libm's pow in the reference: here binary64 sqrt
// for PER_alpha = 0.5 (every shipped configuration), the identity for 1, the device pow otherwise -- correctly rounded /
// within an ulp in binary64, i.e. the same float32 except when the binary64 result sits within ~1e-16 (relative) of a
// float32 rounding boundary (probability ~1e-9 per position); tests compare the float32 priorities bit for bit.
#pragma once
#include "mzx_platform.h"
#include "mzx_tree.h"

namespace mzx {

// compute_target_value (replay_buffer.py:230-262) of position `index` of ONE game of T searched positions: rv [T] root
// values, rw / tp [T + 1] reward_history / to_play_history.  The per-position body every operator of this file shares.
MZX_HD inline double n_step_value(const double* rv, const double* rw, const int32_t* tp, const double* discount_pow, int T,
                                  int index, int td_steps) {
  const int me = tp[index];
  const int b = index + td_steps;
  double value = 0.0;
  if (b < T) {
    const double last = tp[b] == me ? rv[b] : -rv[b];
    value = last * discount_pow[td_steps];
  }
  const int stop = b < T ? b : T;       // reward_history[index + 1 : bootstrap_index + 1] has T + 1 entries
  for (int i = 0; index + 1 + i <= stop; ++i) {
    const double r = rw[index + 1 + i];
    const double s = me == tp[index + i] ? r : -r;
    value = value + s * discount_pow[i];
  }
  return value;
}

struct ReplayPriorityOp {
  const double* root_values;    // [G][T]     root.value() of every searched position (0 for an unvisited root)
  const double* rewards;        // [G][T + 1] reward_history (leading 0)
  const int32_t* to_play;       // [G][T + 1] to_play_history
  const double* discount_pow;   // [td_steps + 1] discount ** i, host-computed
  double* targets;              // [G][T] nullable: compute_target_value
  float* priorities;            // [G][T]
  double per_alpha;
  int32_t num_games, moves, td_steps;

  MZX_HD size_t size() const { return (size_t)num_games * moves; }
  MZX_HD void operator()(size_t e) const {
    const int T = moves;
    const int g = (int)(e / T), index = (int)(e % T);
    const double* rv = root_values + (size_t)g * T;
    const double value = n_step_value(rv, rewards + (size_t)g * (T + 1), to_play + (size_t)g * (T + 1), discount_pow, T,
                                      index, td_steps);
    if (targets) targets[e] = value;
    const double gap = fabs(rv[index] - value);
    double p;
    if (per_alpha == 0.5) p = sqrt(gap);
    else if (per_alpha == 1.0) p = gap;
    else p = pow(gap, per_alpha);
    priorities[e] = (float)p;
  }
};

struct ReplayGameMaxOp {       // game_priority = numpy.max(priorities)
  const float* priorities;
  float* game_priority;
  int32_t num_games, moves;
  MZX_HD size_t size() const { return (size_t)num_games; }
  MZX_HD void operator()(size_t g) const {
    const float* p = priorities + g * (size_t)moves;
    float m = p[0];
    for (int i = 1; i < moves; ++i) m = p[i] > m ? p[i] : m;
    game_priority[g] = m;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Device-resident replay store (mzx.replay.DeviceGameStore): finished games live in a RAGGED pool -- a game of T searched
// positions starts at pool row `base` and owns rows base .. base + T, one row per history index (the histories of a
// finished game have T + 1 entries; root_values / child_visits / values have T, their last row is padding):
//   frames [rows][C][H][W] f32, actions [rows] i32, rewards [rows] f64, to_play [rows] i32, root_values [rows] f64 (the
//   reanalysed values when the history carries them), child_visits [rows][A] f64, values [rows] f64 (derived below).

// n-step values of ragged games: compute_target_value for every position of the games (base[g], len[g]) into `values`.
// One wavefront-sized group of 64 elements per game (lane l takes positions l, l + 64, ...), so one launch covers every
// game of an ingest whatever their lengths.
struct ReplayValuesOp {
  const double* root_values;
  const double* rewards;
  const int32_t* to_play;
  const double* discount_pow;   // [td_steps + 1]
  double* values;
  const int64_t* base;          // [num_games]
  const int32_t* len;           // [num_games] T
  int32_t num_games, td_steps;

  MZX_HD size_t size() const { return (size_t)num_games * 64; }
  MZX_HD void operator()(size_t e) const {
    const size_t g = e >> 6;
    const int64_t b = base[g];
    const int T = len[g];
    for (int index = (int)(e & 63); index < T; index += 64)
      values[b + index] = n_step_value(root_values + b, rewards + b, to_play + b, discount_pow, T, index, td_steps);
  }
};

// make_target (replay_buffer.py:264-303) and the gradient scale (:103-111) of a batch: one element per (sample, unroll
// step).  Inside the game the stored value / reward / child visits / action; at index T value 0, the stored reward, the
// uniform policy, the stored action; past T (absorbing steps) zeros, the uniform policy and the action the HOST drew
// (numpy.random.choice(action_space), :301 -- the draws stay numpy's).  Everything stays binary64 / integer: copies only,
// the uniform probability is the Python expression 1 / A.
struct ReplayTargetsOp {
  const int32_t* actions;
  const double* rewards;
  const double* child_visits;
  const double* values;
  const int64_t* base;            // [n]
  const int32_t* len;             // [n] T
  const int32_t* pos;             // [n]
  const int32_t* absorbing;       // [n][U + 1]
  double* value;                  // [n][U + 1]
  double* reward;                 // [n][U + 1]
  double* policy;                 // [n][U + 1][A]
  int64_t* action;                // [n][U + 1]
  int64_t* gradient_scale;        // [n][U + 1]
  int32_t n, U, A;

  MZX_HD size_t size() const { return (size_t)n * (U + 1); }
  MZX_HD void operator()(size_t e) const {
    const int s = (int)(e / (size_t)(U + 1));
    const int T = len[s], p = pos[s];
    const int idx = p + (int)(e % (size_t)(U + 1));
    const int64_t row = base[s] + (idx < T ? idx : T);
    double* pol = policy + e * (size_t)A;
    if (idx < T) {
      value[e] = values[row];
      const double* cv = child_visits + row * A;
      for (int a = 0; a < A; ++a) pol[a] = cv[a];
    } else {
      value[e] = 0.0;
      const double uniform = 1.0 / (double)A;
      for (int a = 0; a < A; ++a) pol[a] = uniform;
    }
    reward[e] = idx <= T ? rewards[row] : 0.0;
    action[e] = idx <= T ? actions[row] : absorbing[e];
    const int left = T + 1 - p;      // len(action_history) - game_pos
    gradient_scale[e] = U < left ? U : left;
  }
};

// The reanalyse sweep (DeviceGameStore.reanalyse): the positions of G ragged games, flattened in game order, as the sample
// list mzx_replay_batch_io takes -- element e is flat position `first_position + e`; `first` [G] is the exclusive prefix
// of `len` (the caller's only per-sweep host work is O(games)).  The game of a flat position is the LAST g with
// first[g] <= position: games of T == 0 share their first with the next game and are passed over.
struct ReplayPositionsOp {
  const int64_t* base;          // [num_games]
  const int32_t* len;           // [num_games] T
  const int64_t* first;         // [num_games] exclusive prefix of len
  int64_t* sample_base;         // [count]
  int32_t* sample_len;          // [count]
  int32_t* sample_pos;          // [count]
  int64_t first_position;
  int32_t num_games, count;

  MZX_HD size_t size() const { return (size_t)count; }
  MZX_HD void operator()(size_t e) const {
    const int64_t p = first_position + (int64_t)e;
    int lo = 0, hi = num_games - 1;      // first[lo] <= p always (first[0] == 0)
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (first[mid] <= p) lo = mid; else hi = mid - 1;
    }
    sample_base[e] = base[lo];
    sample_len[e] = len[lo];
    sample_pos[e] = (int32_t)(p - first[lo]);
  }
};

// Value logits [n][2 * support_size + 1] of a chunk of such samples -> the decoded root values (SupportToScalarOp's
// function: the float32 bits of mzx_support_to_scalar) into out [n] and, widened to binary64 -- what float(v) of the
// downloaded float32 uploads on the per-game path --, into the pool's root_values row of every sample.
struct ReplayReanalyseOp {
  const float* logits;
  const int64_t* sample_base;   // [n]
  const int32_t* sample_pos;    // [n]
  float* out;                   // [n]
  double* root_values;          // the pool column
  int32_t n, support_size;

  MZX_HD size_t size() const { return (size_t)n; }
  MZX_HD void operator()(size_t e) const {
    const float v = support_to_scalar(logits + (int64_t)e * (2 * support_size + 1), support_size);
    out[e] = v;
    root_values[sample_base[e] + sample_pos[e]] = (double)v;
  }
};

}  // namespace mzx
