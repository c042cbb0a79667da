// mzx_resident.h -- RESIDENT rounds of a slot group (mzx_actor_set_resident): the group's games (mzx_games_device.h), its
// move log and its per-slot bookkeeping live on the device, and mzx_selfplay_rounds queues whole rounds back to back --
// draws -> search -> action choice + vote -> commit -- without an upload, a download or a wait in between.  The host
// comes back once per CHUNK of rounds to collect the games that finished.  Same games, field for field, as the host loop of
// mzx_actor.h on device draws (tests/resident_rounds_cases.py).
//
// Device state of a group (one allocation):
//   start [B] i64, temps [B] f64            the round a slot's game began in, the temperature it began under
//   log rows [cap][B], cap = max_moves + chunk + 1, row (round % cap): observation searched [E] f32, to_play i32, action
//                                           i64, visit_counts [A] i32, root value f64, reward f64, legal mask [A] u8 (games
//                                           whose legal sets vary).  A finished game's rows are read at the end of its
//                                           chunk, at most chunk - 1 rounds after its last one: never overwritten before
//   finished [chunk][B]                     length of the game slot s ended in round q of the chunk (0: none), its terminal
//                                           observation [E] and side to move (self_play.py:166-168) -- one cell per (round,
//                                           slot), so the list needs no counter and comes out in (round, slot) order
//   control block                           [0] halt word (info flag bits), [1] round of the chunk that halted (-1: none)
//
// The halt rule.  A search whose tree raised an info flag (tape overflow: a longer tape is needed; node overflow: an error)
// must not be committed -- and neither may any later round, which would search positions that do not exist yet.  The vote
// (behind the action choice) ORs the flags of its round into the halt word with an ordinary atomic; commit does nothing
// while the word is set.  Commit is a launch of its own behind the vote: the decision is group-wide, and no game may step
// in a round in which ANY tree of the group was flagged -- the host repairs the round as a whole.  After a halt at round r
// the device state is the state before round r; the rounds queued behind it were no-ops (their draws and searches ran and
// are discarded: their counters are not consumed).
#pragma once
#include <algorithm>

#include "mzx_actor.h"
#include "mzx_games_device.h"

namespace mzx {

struct ResidentDevice {
  GameView game;
  int32_t B = 0, A = 0, E = 0, max_moves = 0, chunk = 0, masks = 0;
  int64_t cap = 0;
  int64_t* start = nullptr;
  double* temps = nullptr;
  float* l_obs = nullptr;
  int32_t* l_tp = nullptr;
  int64_t* l_act = nullptr;
  int32_t* l_vis = nullptr;
  double* l_val = nullptr;
  double* l_rew = nullptr;
  uint8_t* l_mask = nullptr;
  int32_t* ctrl = nullptr;            // [4]; fin_len follows it (one download brings both)
  int32_t* fin_len = nullptr;         // [chunk][B]
  int32_t* fin_tp = nullptr;          // [chunk][B]
  float* fin_obs = nullptr;           // [chunk][B][E]
  // the move's device blocks: what the next search reads, what the last one wrote
  float* in_obs = nullptr;
  int32_t* in_legal = nullptr;
  int32_t* in_to_play = nullptr;
  double* in_temperature = nullptr;
  const int32_t* visits = nullptr;
  const double* root_value = nullptr;
  const int64_t* action = nullptr;
  const int32_t* info = nullptr;
};

constexpr int RESIDENT_CTRL_WORDS = 4;

// The vote of round q of the chunk: WAVE_LANES trees per work item.
struct ResidentVoteBody {
  ResidentDevice d;
  int32_t q;
  MZX_HD size_t size() const { return (size_t)((d.B + WAVE_LANES - 1) / WAVE_LANES); }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int32_t halted = d.ctrl[1];
    if (halted >= 0 && halted != q) return;          // an earlier round halted: this one searched nothing that exists
    const int k = (int)e * WAVE_LANES + lane;
    if (k >= d.B) return;
    const int32_t flags = d.info[4 * k + 1];
    if (flags != 0) {
      d.ctrl[1] = q;                                   // (every flagged tree of the launch stores the same round)
      wave_atomic_or(&d.ctrl[0], flags);
    }
  }
};

// Commit of round r (round q of the chunk): one game per wavefront.  prime: only the inputs of the first search.
struct ResidentCommitBody {
  ResidentDevice d;
  int64_t r;
  int32_t q, prime, temperature_threshold;
  double temperature;                  // of the games that start during the call
  MZX_HD size_t size() const { return (size_t)d.B; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    if (d.ctrl[0] != 0) return;
    const int s = (int)e, A = d.A, E = d.E, B = d.B;
    const GameView& v = d.game;
    int64_t start = d.start[s];
    double temp = d.temps[s];
    if (!prime) {
      const size_t row = (size_t)(r % d.cap) * B + s;
      const int64_t action = d.action[s];
      WAVE_FOR(j, E) d.l_obs[row * E + j] = d.in_obs[(size_t)s * E + j];
      WAVE_FOR(j, A) d.l_vis[row * A + j] = d.visits[(size_t)s * A + j];
      if (d.masks) {                   // the legal set the row was searched under: what the legal row was compacted from
        const int8_t* b = v.board + (size_t)s * v.rows * v.cols;
        WAVE_FOR(j, A) d.l_mask[row * A + j] = kin_action_free(v, b, j) ? 1 : 0;
      }
      if (lane == 0) {
        d.l_tp[row] = d.in_to_play[s];
        d.l_act[row] = action;
        d.l_val[row] = d.root_value[s];
      }
      double reward = 0.0;
      uint8_t done = 0;
      if (action >= 0 && action < A) game_wave_step(v, s, lane, action, &reward, &done);
      if (lane == 0) d.l_rew[row] = reward;
      if ((r - start) + 2 > d.max_moves) done = 1;        // len(action_history) <= max_moves, self_play.py:129
      wave_fence();                    // the stone lane 0 stored is read by every lane below
      const size_t cell = (size_t)q * B + s;
      if (done) {
        // the position after the last move closes the record (self_play.py:166-168); the slot's next game begins
        game_wave_position(v, s, lane, d.fin_obs + cell * E, nullptr, d.fin_tp + cell);
        wave_fence();
        game_wave_reset(v, s, lane);
        wave_fence();
        const int32_t length = (int32_t)(r - start + 1);
        start = r + 1;
        temp = temperature;
        if (lane == 0) { d.fin_len[cell] = length; d.start[s] = start; d.temps[s] = temp; }
      } else if (lane == 0) {
        d.fin_len[cell] = 0;
      }
    }
    // the next search's inputs, straight into the move's input block; its temperature (self_play.py:151-157)
    game_wave_position(v, s, lane, d.in_obs + (size_t)s * E, d.in_legal + (size_t)s * A, d.in_to_play + s);
    const int64_t moves_before = (prime ? r : r + 1) - start;
    if (lane == 0)
      d.in_temperature[s] = (temperature_threshold && moves_before + 1 >= temperature_threshold) ? 0.0 : temp;
  }
};

// Finished games packed game-major and ragged, in the layout of mzx_actor::Batch: one game per wavefront.
struct ResidentGatherBody {
  ResidentDevice d;
  const int64_t* table;                // [count][5]: first round, slot, length, offset in the (n + 1)-long arrays, in the n-long
  int32_t count, q_first;              // (q of a game = its last round - r_first + q_first)
  int64_t r_first;
  float* obs; int64_t* act; int64_t* tp; double* rew; int32_t* vis; double* val; uint8_t* mask;
  MZX_HD size_t size() const { return (size_t)count; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t* t = table + 5 * e;
    const int64_t st = t[0], s = t[1], n = t[2], q1 = t[3], q0 = t[4];
    const int A = d.A, E = d.E, B = d.B;
    if (lane == 0) { act[q1] = 0; rew[q1] = 0.0; }      // action_history / reward_history start with 0 (self_play.py:118-120)
    for (int64_t m = 0; m < n; ++m) {
      const size_t row = (size_t)((st + m) % d.cap) * B + (size_t)s;
      WAVE_FOR(j, E) obs[(size_t)(q1 + m) * E + j] = d.l_obs[row * E + j];
      WAVE_FOR(j, A) vis[(size_t)(q0 + m) * A + j] = d.l_vis[row * A + j];
      if (mask) WAVE_FOR(j, A) mask[(size_t)(q0 + m) * A + j] = d.l_mask[row * A + j];
      if (lane == 0) {
        tp[q1 + m] = d.l_tp[row];
        act[q1 + m + 1] = d.l_act[row];
        rew[q1 + m + 1] = d.l_rew[row];
        val[q0 + m] = d.l_val[row];
      }
    }
    const size_t cell = (size_t)((st + n - 1 - r_first) + q_first) * B + (size_t)s;
    WAVE_FOR(j, E) obs[(size_t)(q1 + n) * E + j] = d.fin_obs[cell * E + j];
    if (lane == 0) tp[q1 + n] = d.fin_tp[cell];
  }
};

}  // namespace mzx

// the host side of a resident group
struct mzx_actor_resident {
  mzx::ResidentDevice d;
  mzx_game_device* game = nullptr;
  void* block = nullptr;
  int64_t block_bytes = 0;
  bool primed = false;
  std::vector<int32_t> h_ctrl;         // control block + finished lengths, as downloaded
  void* d_pack = nullptr;              // gather table + packed arrays (grown on demand)
  int64_t pack_bytes = 0;
  int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
