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
#include "mzx_wave.h"

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

// |root - target| ** PER_alpha in binary64 (replay_buffer.py:44): sqrt for 0.5 (every shipped configuration), the identity
// for 1, pow otherwise.  The one statement of it: mzx_replay_priorities and the bulk ingest both go through here.
MZX_HD inline double priority_of_gap(double gap, double per_alpha) {
  if (per_alpha == 0.5) return sqrt(gap);
  if (per_alpha == 1.0) return gap;
  return pow(gap, per_alpha);
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
    priorities[e] = (float)priority_of_gap(fabs(rv[index] - value), per_alpha);
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
// game of an ingest whatever their lengths.  The bulk ingest (mzx_replay_ingest) runs the same operator with `priorities`
// set: the initial PER priority of every position, (float)priority_of_gap(|root - value|), goes to the sampler's column next
// to the value; and with `rows` set a game whose rows would leave the pool is passed over.
struct ReplayValuesOp {
  const double* root_values;
  const double* rewards;
  const int32_t* to_play;
  const double* discount_pow;   // [td_steps + 1]
  double* values;
  const int64_t* base;          // [num_games]
  const int32_t* len;           // [num_games] T
  float* priorities = nullptr;  // the sampler's column, or null
  double per_alpha = 0.0;
  int64_t rows = 0;             // > 0: the pool's row count, checked per game
  int32_t num_games, td_steps;

  MZX_HD size_t size() const { return (size_t)num_games * 64; }
  MZX_HD void operator()(size_t e) const {
    const size_t g = e >> 6;
    const int64_t b = base[g];
    const int T = len[g];
    if (rows > 0 && (b < 0 || T < 0 || b + T >= rows)) return;
    for (int index = (int)(e & 63); index < T; index += 64) {
      const double value = n_step_value(root_values + b, rewards + b, to_play + b, discount_pow, T, index, td_steps);
      values[b + index] = value;
      if (priorities) priorities[b + index] = (float)priority_of_gap(fabs(root_values[b + index] - value), per_alpha);
    }
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

// ---------------------------------------------------------------------------------------------------------------------
// Prioritised sampling and priority feedback on the device (mzx_replay_sampler, include/mzx.h): the store also holds the
// PER priorities -- `priorities` f32 [rows], row base + i the priority of position i < T, the padding row base + T 0 -- and
// a table of `slots` games, slot = game_id % slots: slot_game i64 (-1: empty), slot_base i64, slot_len i32, slot_priority
// f32 (the maximum of the game's priorities: game_priority), slot_sum f64 (their sum).
//
// The draw (mzx_replay_sample) is the reference's two-level one -- game by game_priority, position by priorities,
// replay_buffer.py:166-202 -- stated over a counter-based generator so that sample i of call c is a pure function of
// (seed, c, i): Philox4x32-10, key = the halves of the seed, counter = (i, c lo, c hi, block).  Block 0 gives the two
// uniforms (53 bits each), blocks 1, 2, ... one word per unroll step for the absorbing actions.
// A weight is the float32 priority widened to binary64; a non-finite or non-positive one counts as 0.  At each level the
// target is t = u * total and the draw is the smallest index whose inclusive prefix exceeds t (strictly), where the
// prefix is accumulated in binary64: slots in tiles of 256 (per-tile sums, a prefix over the tiles, a scan inside the
// chosen tile), positions in chunks of 256 with a running carry.  If rounding leaves no such index the last index of
// positive weight is taken; a level whose total is 0 is drawn uniformly (over live games / over the T positions).
// Importance weight: raw = 1 / ((total_samples * (w_s / S)) * (p_i / P)), weight = float32(raw / max raw) -- binary64
// throughout (the reference divides by the maximum in float32: this opt-in path defines its own rounding); a sample drawn
// while no game is live, and every sample when total_samples <= 0, gets the weight 0.
//
// Wave bodies (mzx_wave.h): a wavefront per refreshed game / per tile / per sample in the product build, the same bodies
// with one lane in the tests/hostcheck build.  The sums of one build are always taken in the same association, so a run
// repeats bit for bit; the two builds associate differently and agree exactly wherever the sums are exact.
constexpr int SAMPLER_TILE = 256;

MZX_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// 53 random bits -> [0, 1): ((hi << 21) | (lo >> 11)) * 2^-53
MZX_HD inline double sampler_u53(uint32_t hi, uint32_t lo) {
  return (double)(((uint64_t)hi << 21) | (uint64_t)(lo >> 11)) * (1.0 / 9007199254740992.0);
}
MZX_HD inline double sampler_weight(float p) { return (p > 0.0f && p <= 3.402823466e+38f) ? (double)p : 0.0; }

struct ReplaySamplerTable {
  float* priorities;            // [rows]
  int32_t* owner;               // [rows] scratch of the scatter: -1 between calls
  const int64_t* slot_game;     // [slots]
  const int64_t* slot_base;
  const int32_t* slot_len;
  float* slot_priority;
  double* slot_sum;
  int64_t rows;
  int32_t slots;

  // a slot whose game lies inside the pool (an entry that does not is never followed)
  MZX_HD bool resident(int s) const {
    const int64_t b = slot_base[s];
    const int64_t T = slot_len[s];
    return slot_game[s] >= 0 && b >= 0 && T >= 0 && b + T < rows;
  }
  // kind 0: game_priority; kind 1: 1 for every game that has a position
  MZX_HD double weight(int s, int kind) const {
    if (s >= slots || !resident(s) || slot_len[s] < 1) return 0.0;
    return kind == 0 ? sampler_weight(slot_priority[s]) : 1.0;
  }
  MZX_HD int slot_of(int64_t game_id) const {
    if (game_id < 0) return -1;
    const int s = (int)(game_id % slots);
    return slot_game[s] == game_id && resident(s) ? s : -1;
  }
};

struct ReplayRefreshParams {
  ReplaySamplerTable t;
  const int32_t* slot_list;     // [n], or
  const int64_t* game_ids;      // [n]: the slots of these games; one that left the table is passed over
  int32_t n;
  MZX_HD int slot(size_t e) const {
    if (!slot_list) return t.slot_of(game_ids[e]);
    const int s = slot_list[e];
    return s >= 0 && s < t.slots ? s : -1;
  }
};

struct ReplayDrawParams {
  ReplaySamplerTable t;
  double* tile_prefix;          // [2][tiles] inclusive prefix of the tile sums: kind 0, then kind 1
  double* raw;                  // [n] (per only)
  const int32_t* action_space;  // [A] nullable: the identity
  const double* uniforms;       // [n][2] nullable
  int64_t* out_base;
  int32_t* out_len;
  int32_t* out_pos;
  int32_t* out_tape;            // [n][U + 1]
  int64_t* out_game;
  float* out_weight;            // [n] (per only)
  uint64_t seed, call_counter;
  int64_t total_samples;
  int32_t n, per, U, A, tiles;

  MZX_HD void block(int i, uint32_t j, uint32_t w[4]) const {
    philox4x32_10((uint32_t)i, (uint32_t)call_counter, (uint32_t)(call_counter >> 32), j, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  }
  MZX_HD void uniform_pair(int i, double& u_game, double& u_pos) const {
    if (uniforms) {
      u_game = uniforms[2 * (size_t)i];
      u_pos = uniforms[2 * (size_t)i + 1];
      return;
    }
    uint32_t w[4];
    block(i, 0, w);
    u_game = sampler_u53(w[0], w[1]);
    u_pos = sampler_u53(w[2], w[3]);
  }
  // kind of the game level: the priorities, or every live game alike (PER off, or no positive priority anywhere)
  MZX_HD int kind() const { return per && tile_prefix[tiles - 1] > 0.0 ? 0 : 1; }
  // the tile of target t: the first whose inclusive prefix exceeds it, else the first that reaches the total
  MZX_HD int pick_tile(const double* I, double t) const {
    int lo = 0, hi = tiles;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (I[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo < tiles) return lo;
    const double S = I[tiles - 1];
    lo = 0; hi = tiles - 1;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (I[mid] >= S) hi = mid; else lo = mid + 1;
    }
    return lo;
  }
  MZX_HD int uniform_position(double u, int T) const {
    const double f = floor(u * (double)T);
    return f >= 0.0 ? (f < (double)T ? (int)f : T - 1) : 0;
  }
  // absorbing action of unroll step u of sample i: mulhi(word, A) into the action space
  MZX_HD int32_t absorbing_action(int i, int u) const {
    uint32_t w[4];
    block(i, 1u + (uint32_t)(u >> 2), w);
    const int32_t index = (int32_t)(((uint64_t)w[u & 3] * (uint64_t)(uint32_t)A) >> 32);
    return action_space ? action_space[index] : index;
  }
  MZX_HD void write_sample(int i, int slot, int pos, double w_s, double S, double p_i, double P) const {
    out_base[i] = slot >= 0 ? t.slot_base[slot] : 0;
    out_len[i] = slot >= 0 ? t.slot_len[slot] : 0;
    out_pos[i] = pos;
    out_game[i] = slot >= 0 ? t.slot_game[slot] : -1;
    if (per) raw[i] = slot >= 0 && total_samples > 0 ? 1.0 / (((double)total_samples * (w_s / S)) * (p_i / P)) : 0.0;
  }
};

// The scatter (update_priorities, replay_buffer.py:205-228): sample i writes new[i][k] to position pos_i + k < T of its
// game when the game still holds its slot.  The reference's loop lets the LAST sample win where windows overlap: a claim
// pass takes the integer maximum of i per row (an atomic max: its result does not depend on the order), the write pass
// stores where the claim is its own and puts -1 back.
struct ReplayClaimOp {
  ReplaySamplerTable t;
  const float* fresh;           // [n][steps]
  const int64_t* game_id;       // [n]
  const int32_t* pos;           // [n]
  int32_t n, steps, write;

  MZX_HD size_t size() const { return (size_t)n * steps; }
  MZX_HD void operator()(size_t e) const {
    const int i = (int)(e / (size_t)steps), k = (int)(e % (size_t)steps);
    const int s = t.slot_of(game_id[i]);
    if (s < 0) return;
    const int64_t p = (int64_t)pos[i] + k;
    if (pos[i] < 0 || p >= t.slot_len[s]) return;
    const int64_t row = t.slot_base[s] + p;
    if (!write) {
#ifdef MZX_HOSTCHECK
      if (t.owner[row] < i) t.owner[row] = i;
#else
      atomicMax(t.owner + row, i);
#endif
    } else if (t.owner[row] == i) {
      t.priorities[row] = fresh[e];
      t.owner[row] = -1;
    }
  }
};

constexpr int SAMPLER_WAVES = 4;                                  // wavefronts (games, tiles, samples) per workgroup
constexpr int SAMPLER_PER_LANE = SAMPLER_TILE / WAVE_LANES;       // weights of a tile a lane holds: indices 4l .. 4l + 3 on the device

// maximum and weight sum of the T priorities from row `base` on into slot s (T == 0: 0 / 0): a wavefront's work
MZX_WAVE_FN void refresh_slot(const ReplaySamplerTable& t, int s, int64_t base, int T, int lane) {
  const float* __restrict__ pr = t.priorities + (T ? base : 0);
  float m = -(float)MZX_INF;
  double sum = 0.0;
  WAVE_FOR(i, T) {
    const float v = pr[i];
    if (v > m) m = v;
    sum = sum + sampler_weight(v);
  }
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) {
    const float other = lane_xor(m, o);
    if (other > m) m = other;
  }
  sum = wave_sum_f64(sum);
  if (lane == 0) {
    t.slot_priority[s] = T ? m : 0.0f;
    t.slot_sum[s] = sum;
  }
}

// maximum and weight sum of a refreshed game: launch_waves<SAMPLER_WAVES>, a wavefront per game
struct ReplayRefreshBody {
  ReplayRefreshParams p;
  MZX_HD size_t size() const { return (size_t)p.n; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int s = p.slot(e);
    if (s < 0) return;
    refresh_slot(p.t, s, p.t.slot_base[s], p.t.resident(s) ? p.t.slot_len[s] : 0, lane);
  }
};

// the sums of both kinds of weight over a tile of 256 slots: launch_waves<SAMPLER_WAVES>, a wavefront per tile
struct ReplayTileSumBody {
  ReplayDrawParams p;
  MZX_HD size_t size() const { return (size_t)p.tiles; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int k = (int)e;
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int j = 0; j < SAMPLER_PER_LANE; ++j) {
      const int s = k * SAMPLER_TILE + SAMPLER_PER_LANE * lane + j;
      a = a + p.t.weight(s, 0);
      b = b + p.t.weight(s, 1);
    }
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    if (lane == 0) {
      p.tile_prefix[k] = a;
      p.tile_prefix[(size_t)p.tiles + k] = b;
    }
  }
};

// the tile sums -> their inclusive prefix, in place: launch_waves<2>, one workgroup, a wavefront per kind, WAVE_LANES tiles
// per step with a carry
struct ReplayTilePrefixBody {
  ReplayDrawParams p;
  MZX_HD size_t size() const { return 2; }
  MZX_WAVE_FN void operator()(size_t kind, int lane) const {
    double* I = p.tile_prefix + kind * (size_t)p.tiles;
    double carry = 0.0;
    for (int k0 = 0; k0 < p.tiles; k0 += WAVE_LANES) {
      const int k = k0 + lane;
      const double v = wave_scan_f64(k < p.tiles ? I[k] : 0.0, lane);
      if (k < p.tiles) I[k] = carry + v;
      carry = carry + lane_value(v, WAVE_LANES - 1);
    }
  }
};

// One level of a draw over the 256 weights of a tile, SAMPLER_PER_LANE per lane: the first index whose carry + inclusive
// prefix exceeds t and whose weight is positive (-1: none), `last` the last index of positive weight (-1: none), `total`
// the sum of the 256.  The same value in every lane.
MZX_WAVE_FN int wave_pick(const double w[SAMPLER_PER_LANE], double carry, double t, int lane, int& last, double& total) {
  constexpr int N = SAMPLER_PER_LANE;
  double run[N];                     // the lane's own inclusive prefix
  run[0] = w[0];
#pragma unroll
  for (int j = 1; j < N; ++j) run[j] = run[j - 1] + w[j];
  const double incl = wave_scan_f64(run[N - 1], lane);
  double below = lane_up(incl, 1);
  if (lane == 0) below = 0.0;
  total = lane_value(incl, WAVE_LANES - 1);
  int first = -1, tail = -1;
#pragma unroll
  for (int j = N - 1; j >= 0; --j) if (w[j] > 0.0 && carry + (below + run[j]) > t) first = j;
#pragma unroll
  for (int j = 0; j < N; ++j) if (w[j] > 0.0) tail = j;
  const int first_lane = wave_first_lane(first >= 0), tail_lane = wave_last_lane(tail >= 0);
  const int first_j = lane_value(first, first_lane < 0 ? 0 : first_lane), tail_j = lane_value(tail, tail_lane < 0 ? 0 : tail_lane);
  last = tail_lane < 0 ? -1 : N * tail_lane + tail_j;
  return first_lane < 0 ? -1 : N * first_lane + first_j;
}

// One sample of a draw: launch_waves<SAMPLER_WAVES>, a wavefront per sample
struct ReplayDrawBody {
  ReplayDrawParams p;
  MZX_HD size_t size() const { return (size_t)p.n; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    constexpr int N = SAMPLER_PER_LANE;
    const int i = (int)e;
    double u_game = 0.0, u_pos = 0.0;
    if (lane == 0) p.uniform_pair(i, u_game, u_pos);                  // lane 0's Philox block, broadcast
    u_game = lane_value(u_game, 0);
    u_pos = lane_value(u_pos, 0);

    const int kind = p.kind();
    const double* __restrict__ I = p.tile_prefix + (size_t)kind * p.tiles;
    const double S = I[p.tiles - 1];
    int slot = -1, last;
    double total, w[N];
    if (S > 0.0) {
      const double t = u_game * S;
      const int k = p.pick_tile(I, t);
#pragma unroll
      for (int j = 0; j < N; ++j) w[j] = p.t.weight(k * SAMPLER_TILE + N * lane + j, kind);
      int j = wave_pick(w, k ? I[k - 1] : 0.0, t, lane, last, total);
      if (j < 0) j = last;
      if (j >= 0) slot = k * SAMPLER_TILE + j;
      for (int k2 = p.tiles - 1; k2 >= 0 && slot < 0; --k2) {          // (a table whose prefix misled the search: its last live slot)
#pragma unroll
        for (int j2 = 0; j2 < N; ++j2) w[j2] = p.t.weight(k2 * SAMPLER_TILE + N * lane + j2, kind);
        wave_pick(w, 0.0, 0.0, lane, last, total);
        if (last >= 0) slot = k2 * SAMPLER_TILE + last;
      }
    }
    const int T = slot >= 0 ? p.t.slot_len[slot] : 0;
    const float* __restrict__ pr = p.t.priorities + (slot >= 0 ? p.t.slot_base[slot] : 0);
    int pos = -1;
    double p_i = 1.0, P = (double)T;
    const double sum = slot >= 0 ? p.t.slot_sum[slot] : 0.0;
    if (p.per && sum > 0.0 && sum <= 1.7976931348623157e308) {
      const double t = u_pos * sum;
      double carry = 0.0;
      int seen = -1;
      for (int c0 = 0; c0 < T && pos < 0; c0 += SAMPLER_TILE) {        // (pos is the same in every lane)
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const int idx = c0 + N * lane + j;
          w[j] = idx < T ? sampler_weight(pr[idx]) : 0.0;
        }
        const int j = wave_pick(w, carry, t, lane, last, total);
        if (last >= 0) seen = c0 + last;
        if (j >= 0) pos = c0 + j;
        carry = carry + total;
      }
      if (pos < 0) pos = seen;
      if (pos >= 0) {
        p_i = sampler_weight(pr[pos]);
        P = sum;
      }
    }
    if (pos < 0) pos = T > 0 ? p.uniform_position(u_pos, T) : 0;
    if (lane == 0) p.write_sample(i, slot, pos, slot >= 0 ? p.t.weight(slot, kind) : 0.0, S, p_i, P);
    WAVE_FOR(u, p.U + 1) p.out_tape[(size_t)i * (p.U + 1) + u] = u >= T + 1 - pos ? p.absorbing_action(i, u) : 0;
  }
};

// weight = float32(raw / max raw): launch_block<SAMPLER_FINISH_BLOCK>
constexpr int SAMPLER_FINISH_BLOCK = 256;
struct ReplayWeightFinishBody {
  ReplayDrawParams p;
  MZX_WAVE_FN void operator()(int t) const {
    constexpr int THREADS = block_threads(SAMPLER_FINISH_BLOCK);
    MZX_BLOCK_SHARED double part[THREADS];
    double m = -MZX_INF;
    for (int i = t; i < p.n; i += THREADS) if (p.raw[i] > m) m = p.raw[i];
    part[t] = m;
    block_sync();
    for (int o = THREADS / 2; o >= 1; o >>= 1) {
      if (t < o && part[t + o] > part[t]) part[t] = part[t + o];
      block_sync();
    }
    m = part[0];
    for (int i = t; i < p.n; i += THREADS) p.out_weight[i] = m > 0.0 ? (float)(p.raw[i] / m) : 0.0f;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Reanalyse with fresh searches (DeviceGameStore.reanalyse_search): a chunk of the sweep's sample list (ReplayPositionsOp)
// becomes the inputs of one mzx_search_run, and the chunk's search outputs become the policy and root-value targets of the
// pool, in place.  Two wave bodies, launch_waves<SAMPLER_WAVES>, a wavefront per sample.
//
// The optional legal-mask column is u32 [rows][ceil(A / 32)], bit a % 32 of word a / 32 set when action a is legal at that
// row; bits past A are ignored.  The roots see their legal actions in INCREASING action order.
// Tie-break tape: Philox4x32-10 under the key (seed lo, seed hi ^ "REAS") -- apart from the sampler's stream --, counter
// (position's index in the sweep, sweep counter lo, hi, block); block b supplies words 4b .. 4b + 3 of the sample's row.
constexpr uint32_t REANALYSE_SEARCH_KEY = 0x52454153u;
constexpr int32_t SEARCH_INPUT_EMPTY_MASK = 1;     // d_input_flags: the mask row had no bit set (the identity list is searched)
constexpr int32_t SEARCH_INPUT_BAD_ROW = 2;        // the sample's row lies outside the pool (nothing of the pool is read)

MZX_HD inline int mask_popcount(uint32_t w) { return __builtin_popcount(w); }
// word w of a mask row with the bits of actions >= A cleared
MZX_HD inline uint32_t mask_word(const uint32_t* m, int w, int A) {
  const int left = A - 32 * w;
  return left >= 32 ? m[w] : m[w] & ((1u << left) - 1u);
}

struct ReplaySearchInputsBody {
  const int32_t* pool_to_play;  // the pool column
  const uint32_t* legal_mask;   // [rows][mask_words] nullable: every action legal
  const int64_t* sample_base;   // [n]
  const int32_t* sample_pos;    // [n]
  int32_t* to_play;             // [n]
  int32_t* legal;               // [n][A]
  uint32_t* tape;               // [n][tape_words]
  int32_t* flags;               // [n]
  uint64_t seed, sweep_counter;
  int64_t first_index, rows;
  int32_t n, A, tape_words;

  MZX_HD size_t size() const { return (size_t)n; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t row = sample_base[e] + sample_pos[e];
    const bool inside = row >= 0 && row < rows;
    const int words = (A + 31) / 32;
    const uint32_t* __restrict__ m = legal_mask && inside ? legal_mask + row * words : nullptr;
    int count = 0;                                     // (every lane counts the few words of the row itself)
    if (m) for (int w = 0; w < words; ++w) count += mask_popcount(mask_word(m, w, A));
    int32_t* __restrict__ out = legal + e * (size_t)A;
    if (count == 0) {
      WAVE_FOR(a, A) out[a] = a;
    } else {
      WAVE_FOR(a, A) {
        const int w = a >> 5;
        const uint32_t word = mask_word(m, w, A);
        if ((word >> (a & 31)) & 1u) {                 // its slot: the number of legal actions below it
          int rank = mask_popcount(word & ((1u << (a & 31)) - 1u));
          for (int v = 0; v < w; ++v) rank += mask_popcount(m[v]);
          out[rank] = a;
        }
        if (a >= count) out[a] = -1;
      }
    }
    if (lane == 0) {
      to_play[e] = inside ? pool_to_play[row] : 0;
      flags[e] = !inside ? SEARCH_INPUT_BAD_ROW : (m && count == 0 ? SEARCH_INPUT_EMPTY_MASK : 0);
    }
    const uint64_t index = (uint64_t)first_index + e;
    uint32_t* __restrict__ t = tape + e * (size_t)tape_words;
    WAVE_FOR(b, (tape_words + 3) / 4) {
      uint32_t w[4];
      philox4x32_10((uint32_t)index, (uint32_t)sweep_counter, (uint32_t)(sweep_counter >> 32), (uint32_t)b, (uint32_t)seed,
                    (uint32_t)(seed >> 32) ^ REANALYSE_SEARCH_KEY, w);
      for (int j = 0; j < 4 && 4 * b + j < tape_words; ++j) t[4 * b + j] = w[j];
    }
  }
};

// visits / sum(visits) in binary64 (GameHistory.store_search_statistics, self_play.py:496-511: 0 for an action that is no
// child) and the root value into the pool rows of the samples.  A sample whose search was flagged (info[1]: tie tape or
// node overflow), whose input flag is set or that has no visit keeps both of its rows and counts in skipped[0].
struct ReplaySearchWriteBody {
  const int32_t* visits;        // [n][A]
  const double* root_value;     // [n]
  const int32_t* info;          // [n][4]
  const int32_t* flags;         // [n]
  const int64_t* sample_base;   // [n]
  const int32_t* sample_pos;    // [n]
  double* child_visits;         // the pool columns
  double* root_values;
  int32_t* skipped;             // [1]
  int32_t n, A;

  MZX_HD size_t size() const { return (size_t)n; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int32_t* __restrict__ v = visits + e * (size_t)A;
    int32_t sum = 0;
    WAVE_FOR(a, A) sum += v[a];
    sum = wave_sum_i32(sum);
    if (info[4 * e + 1] != 0 || flags[e] != 0 || sum < 1) {       // (the same in every lane)
      if (lane == 0) wave_atomic_add(skipped, 1);
      return;
    }
    const int64_t row = sample_base[e] + sample_pos[e];
    double* __restrict__ cv = child_visits + row * A;
    const double total = (double)sum;
    WAVE_FOR(a, A) cv[a] = (double)v[a] / total;
    if (lane == 0) root_values[row] = root_value[e];
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Bulk ingest (mzx_replay_ingest, include/mzx.h): the finished games of a hand-off, staged game-major and ragged as the
// shard's records hold them, become pool rows.  Three launches whatever the number of games: ReplayIngestRowBody (a
// wavefront per pool row), ReplayValuesOp with the priority column, ReplayIngestSlotBody (a wavefront per game).
// Staged row r of the arrays with T + 1 entries per game belongs to the LAST game g with src1[g] <= r (src1 is strictly
// increasing: every game has its padding row), index i = r - src1[g]; its row of the arrays with T entries is src0[g] + i.

// a 16-byte group of a frame, and a load of staged data that is read once (non-temporal on the device)
#ifdef MZX_HOSTCHECK
struct f32x4 { float v[4]; };
template <class T> inline T load_once(const T* p) { return *p; }
#else
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <class T> __device__ __forceinline__ T load_once(const T* p) { return __builtin_nontemporal_load(p); }
#endif

struct ReplayIngestParams {
  const int32_t* len;           // [G]
  const int64_t* base;          // [G]
  const int64_t* game_id;       // [G]
  const int64_t* src1;          // [G]
  const int64_t* src0;          // [G]
  const float* observations;    // staged, see include/mzx.h
  const int64_t* actions;
  const double* rewards;
  const int64_t* to_play;
  const int32_t* visits;
  const double* root_values;
  const uint8_t* legal;         // nullable
  const float* staged_priorities;   // nullable
  float* pool_frames;           // the pool's columns
  int32_t* pool_actions;
  double* pool_rewards;
  int32_t* pool_to_play;
  double* pool_root_values;
  double* pool_child_visits;
  uint32_t* pool_mask;          // nullable
  float* pool_priorities;       // nullable: no sampler
  int64_t rows, total_rows;
  int32_t G, A, frame_floats, vec, per;
};

struct ReplayIngestRowBody {
  ReplayIngestParams p;
  MZX_HD size_t size() const { return (size_t)p.total_rows; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t r = (int64_t)e;
    int lo = 0, hi = p.G - 1;            // src1[lo] <= r always (src1[0] == 0); the same search in every lane
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (p.src1[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int g = lo;
    const int T = p.len[g];
    const int64_t i = r - p.src1[g], b = p.base[g];
    if (i < 0 || i > T || b < 0 || b + T >= p.rows) return;      // (an entry that leaves the pool is never followed)
    const int64_t row = b + i;
    const bool inside = i < T;
    const int A = p.A;

    // the frame: 16 bytes per lane and step where the row size and both addresses allow it, a dword otherwise
    if (p.vec) {
      const f32x4* __restrict__ src = (const f32x4*)(p.observations + r * p.frame_floats);
      f32x4* __restrict__ dst = (f32x4*)(p.pool_frames + row * p.frame_floats);
      WAVE_FOR(j, p.frame_floats / 4) dst[j] = load_once(src + j);
    } else {
      const float* __restrict__ src = p.observations + r * p.frame_floats;
      float* __restrict__ dst = p.pool_frames + row * p.frame_floats;
      WAVE_FOR(j, p.frame_floats) dst[j] = load_once(src + j);
    }

    // child visits: visits / their sum, 0 for an illegal action, an unvisited root and the padding row
    const int64_t r0 = p.src0[g] + i;
    const int32_t* __restrict__ v = p.visits + r0 * A;
    const uint8_t* __restrict__ ok = p.legal && inside ? p.legal + r0 * A : nullptr;
    int32_t sum = 0;
    if (inside) WAVE_FOR(a, A) sum += load_once(v + a);
    sum = wave_sum_i32(sum);
    const double total = (double)sum;
    double* __restrict__ cv = p.pool_child_visits + row * A;
    WAVE_FOR(a, A) cv[a] = inside && sum > 0 && (!ok || ok[a]) ? (double)v[a] / total : 0.0;

    // the legal-mask column: a lane per word
    if (p.pool_mask) {
      const int words = (A + 31) / 32;
      uint32_t* __restrict__ m = p.pool_mask + row * words;
      WAVE_FOR(w, words) {
        uint32_t word = 0xFFFFFFFFu;
        if (ok) {
          word = 0;
          for (int a = 32 * w; a < A && a < 32 * w + 32; ++a) word |= ok[a] ? 1u << (a & 31) : 0u;
        }
        m[w] = word;
      }
    }

    if (lane == 0) {
      p.pool_actions[row] = (int32_t)load_once(p.actions + r);
      p.pool_rewards[row] = load_once(p.rewards + r);
      p.pool_to_play[row] = (int32_t)load_once(p.to_play + r);
      p.pool_root_values[row] = inside && sum > 0 ? load_once(p.root_values + r0) : 0.0;
      if (p.pool_priorities) {
        if (!inside || !p.per) p.pool_priorities[row] = 0.0f;
        else if (p.staged_priorities) p.pool_priorities[row] = load_once(p.staged_priorities + r0);
      }                                   // (per without staged priorities: the values launch writes them)
    }
  }
};

// the table slots of the ingested games and their maximum / sum: launch_waves<SAMPLER_WAVES>, a wavefront per game
struct ReplayIngestSlotBody {
  ReplaySamplerTable t;
  int64_t* slot_game;           // the table's columns, writable
  int64_t* slot_base;
  int32_t* slot_len;
  const int64_t* game_id;       // [n]
  const int64_t* base;
  const int32_t* len;
  int32_t n;
  MZX_HD size_t size() const { return (size_t)n; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t id = game_id[e], b = base[e];
    const int T = len[e];
    if (id < 0 || b < 0 || T < 0 || b + T >= t.rows) return;      // (as the other two launches: such a game is passed over)
    const int s = (int)(id % t.slots);
    if (lane == 0) {
      slot_game[s] = id;
      slot_base[s] = b;
      slot_len[s] = T;
    }
    refresh_slot(t, s, b, T, lane);
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Export (mzx_replay_export, include/mzx.h): the inverse of the ingest's row launch, for reading games back.  Games
// (base[g], len[g]) of the pool are packed game-major and ragged in the ingest's staged layout: packed row r of the arrays
// with T + 1 entries per game belongs to the LAST game g with dst1[g] <= r, index i = r - dst1[g]; its row of the arrays
// with T entries is dst0[g] + i.  One launch, a wavefront per packed row; copies only -- the child visits are the pool's
// quotients as they lie, actions / to_play widened to i64, a mask row expanded to one byte per action.
struct ReplayExportParams {
  const int64_t* base;          // [G]
  const int32_t* len;           // [G]
  const int64_t* dst1;          // [G]
  const int64_t* dst0;          // [G]
  const float* pool_frames;     // the pool's columns
  const int32_t* pool_actions;
  const double* pool_rewards;
  const int32_t* pool_to_play;
  const double* pool_root_values;
  const double* pool_child_visits;
  const uint32_t* pool_mask;    // null without `legal`
  const float* pool_priorities; // null without `priorities`
  float* observations;          // packed, see include/mzx.h
  int64_t* actions;
  double* rewards;
  int64_t* to_play;
  double* child_visits;
  double* root_values;
  uint8_t* legal;               // nullable
  float* priorities;            // nullable
  int64_t rows, total_rows;
  int32_t G, A, frame_floats, vec;
};

struct ReplayExportRowBody {
  ReplayExportParams p;
  MZX_HD size_t size() const { return (size_t)p.total_rows; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t r = (int64_t)e;
    int lo = 0, hi = p.G - 1;            // dst1[lo] <= r always (dst1[0] == 0); the same search in every lane
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (p.dst1[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int g = lo;
    const int T = p.len[g];
    const int64_t i = r - p.dst1[g], b = p.base[g];
    if (i < 0 || i > T || b < 0 || b + T >= p.rows) return;      // (a game whose rows leave the pool is passed over)
    const int64_t row = b + i;
    const int A = p.A;

    if (p.vec) {
      const f32x4* __restrict__ src = (const f32x4*)(p.pool_frames + row * p.frame_floats);
      f32x4* __restrict__ dst = (f32x4*)(p.observations + r * p.frame_floats);
      WAVE_FOR(j, p.frame_floats / 4) dst[j] = src[j];
    } else {
      const float* __restrict__ src = p.pool_frames + row * p.frame_floats;
      float* __restrict__ dst = p.observations + r * p.frame_floats;
      WAVE_FOR(j, p.frame_floats) dst[j] = src[j];
    }
    if (lane == 0) {
      p.actions[r] = (int64_t)p.pool_actions[row];
      p.rewards[r] = p.pool_rewards[row];
      p.to_play[r] = (int64_t)p.pool_to_play[row];
    }
    if (i == T) return;                  // the padding row has no entry in the arrays of T per game

    const int64_t r0 = p.dst0[g] + i;
    const double* __restrict__ cv = p.pool_child_visits + row * A;
    double* __restrict__ out = p.child_visits + r0 * A;
    WAVE_FOR(a, A) out[a] = cv[a];
    if (p.legal) {
      const uint32_t* __restrict__ m = p.pool_mask + row * ((A + 31) / 32);
      uint8_t* __restrict__ ok = p.legal + r0 * A;
      WAVE_FOR(a, A) ok[a] = (uint8_t)((m[a >> 5] >> (a & 31)) & 1u);
    }
    if (lane == 0) {
      p.root_values[r0] = p.pool_root_values[row];
      if (p.priorities) p.priorities[r0] = p.pool_priorities[row];
    }
  }
};

}  // namespace mzx
