// mzx_games_device.h -- the device-resident twin of a natively stepped game (mzx_games.h): boards, players, keys, step
// counters and seeds of a shard in device memory, stepped, observed and restarted by kernels -- what a round loop that
// never returns to the host per move is built from.
//
// The rules are NOT restated here: the MZX_HD functions of mzx_games.h (the counter hash, the landing cell, "this line is
// won", "this action is free", what an ended game pays) are the ones the host classes call in their per-game loops; the
// wave functions below call them from one wavefront per game (launch_waves, mzx_wave.h): WAVE_FOR over cells, lines and
// observation elements, the legal row compacted in increasing action order by a ballot and a prefix count per
// WAVE_LANES-action pass (gomoku's 121 actions: two passes).  tests/hostcheck (WAVE_LANES = 1) executes the same
// statements serially.  Bit for bit what the host class returns: the synthetic observation is
// (float)((double)h / 4294967296.0) -- an exact binary64 scaling and one IEEE rounding to binary32 on either side --,
// board planes hold -1 / 0 / 1, rewards are small integers in binary64 (tests/test_device_games.py,
// tests/test_gpu_device_games.py).
//
// A move of a board game is judged BEFORE it is stored: every lane reads the board "with my stone on the landing cell"
// (kin_cell) and one lane stores the stone, the player and the outcome afterwards, so no lane depends on another lane's
// store.  Plain vector stores only; no atomics are needed (a wavefront owns its game).
#pragma once
#include "mzx_games.h"
#include "mzx_launch.h"
#include "mzx_wave.h"

struct mzx_game_device {
  mzx::GameView v;              // the arrays below, in device memory
  void* block = nullptr;        // one allocation holds them all
  size_t block_bytes = 0;
};

namespace mzx {

constexpr int GAME_WAVES = 4;   // games per workgroup

// ---- one game per wavefront -------------------------------------------------------------------------------------------

// One move of game g.  reward / done are the same in every lane; the state is stored by lane 0.
MZX_WAVE_FN void game_wave_step(const GameView& v, int g, int lane, int64_t action, double* reward, uint8_t* done) {
  if (v.kind == 0) {
    const uint32_t t = v.t[g] + 1u;
    const uint32_t key = synth_next_key(v.key[g], action, t);
    const int32_t turn = synth_next_turn(v.turn[g], v.num_players);
    if (lane == 0) { v.t[g] = t; v.key[g] = key; v.turn[g] = turn; }
    *reward = synth_reward(key);
    *done = 0;
    return;
  }
  const int cells = v.rows * v.cols;
  int8_t* b = v.board + (size_t)g * cells;
  const int a = (int)action;
  const int8_t me = v.player[g];
  const int cell = kin_landing_cell(v, b, a);
  bool mine = false;
  WAVE_FOR(l, v.num_lines) mine = mine || kin_line_won(v, b, l, cell, me);
  const bool won = wave_ballot(mine) != 0;
  bool open = false;
  WAVE_FOR(j, kin_move_cells(v)) open = open || !kin_move_cell_taken(v, b, j, cell, me);
  const bool no_move = wave_ballot(open) == 0;
  const bool over = won || no_move;
  if (lane == 0) {              // (behind every read of the board above)
    if (cell >= 0) b[cell] = me;
    v.player[g] = (int8_t)-me;
  }
  *done = over ? 1 : 0;
  *reward = kin_reward(v, won, over);
}

// Game g back at its first position.
MZX_WAVE_FN void game_wave_reset(const GameView& v, int g, int lane) {
  if (v.kind == 0) {
    if (lane == 0) { v.t[g] = 0; v.turn[g] = 0; v.key[g] = synth_first_key(v.seeds[g]); }
    return;
  }
  const int cells = v.rows * v.cols;
  int8_t* b = v.board + (size_t)g * cells;
  WAVE_FOR(j, cells) b[j] = 0;
  if (lane == 0) v.player[g] = 1;
}

// The position of game g as the next search reads it: observation row (float32, laid out as mzx_game::observe emits it),
// legal row (increasing, padded with -1) and side to move; each output nullable.  Reads the state only.
MZX_WAVE_FN void game_wave_position(const GameView& v, int g, int lane, float* obs, int32_t* legal, int32_t* to_play) {
  const int A = v.num_actions;
  if (v.kind == 0) {
    if (obs) {
      const uint32_t key = v.key[g];
      WAVE_FOR(j, v.obs_elems) obs[j] = synth_obs_elem(key, j);
    }
    if (legal) WAVE_FOR(a, A) legal[a] = a;
    if (to_play && lane == 0) *to_play = v.turn[g];
    return;
  }
  const int cells = v.rows * v.cols;
  const int8_t* b = v.board + (size_t)g * cells;
  const int8_t player = v.player[g];
  if (obs) {
    WAVE_FOR(j, cells) {
      const int8_t c = b[j];
      for (int plane = 0; plane < 3; ++plane) obs[plane * cells + j] = kin_obs_elem(c, player, plane);
    }
  }
  if (legal) {
    int n = 0;                  // (the same in every lane)
    for (int a0 = 0; a0 < A; a0 += WAVE_LANES) {
      const int a = a0 + lane;
      const bool free_ = a < A && kin_action_free(v, b, a);
      const uint64_t set = wave_ballot(free_);
      if (free_) legal[n + wave_rank_below(set, lane)] = a;      // n + rank < A: at most A actions are free
      n += __builtin_popcountll(set);
    }
    WAVE_FOR(j, A) if (j >= n) legal[j] = -1;
  }
  if (to_play && lane == 0) *to_play = kin_to_play(player);
}

// ---- the kernels of the C entry points --------------------------------------------------------------------------------

struct GameStepBody {
  GameView v;
  const int64_t* actions;       // [B]
  const uint8_t* active;        // [B] nullable
  double* reward;               // [B] nullable
  uint8_t* done;                // [B] nullable
  MZX_HD size_t size() const { return (size_t)v.num_games; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int g = (int)e;
    double r = 0.0;
    uint8_t d = 0;
    // (the synthetic game steps every game, as its Python class does; a board game leaves a finished one untouched.
    //  An action outside the space touches nothing: the host entry cannot see device actions)
    const bool skip = v.kind != 0 && active && !active[g];
    const int64_t a = actions[g];
    if (!skip && a >= 0 && a < v.num_actions) game_wave_step(v, g, lane, a, &r, &d);
    if (lane == 0) {
      if (reward) reward[g] = r;
      if (done) done[g] = d;
    }
  }
};

struct GamePositionBody {
  GameView v;
  float* obs;                   // [B][E] nullable
  int32_t* legal;               // [B][A] nullable
  int32_t* to_play;             // [B] nullable
  MZX_HD size_t size() const { return (size_t)v.num_games; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    game_wave_position(v, (int)e, lane, obs ? obs + e * (size_t)v.obs_elems : nullptr,
                       legal ? legal + e * (size_t)v.num_actions : nullptr, to_play ? to_play + e : nullptr);
  }
};

struct GameResetBody {
  GameView v;
  const int32_t* games;         // [count] nullable: games 0 .. count - 1
  int32_t count;
  MZX_HD size_t size() const { return (size_t)count; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int g = games ? games[e] : (int)e;
    if (g >= 0 && g < v.num_games) game_wave_reset(v, g, lane);      // (a device index list is not the host's to check)
  }
};

// ---- the device object ------------------------------------------------------------------------------------------------

// byte offsets of the arrays inside the one block (each 16-byte aligned); returns the block's size
struct GameDeviceLayout {
  size_t seeds = 0, key = 0, t = 0, turn = 0, board = 0, player = 0, lines = 0, total = 0;
};
inline GameDeviceLayout game_device_layout(const GameView& h) {
  GameDeviceLayout L;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 15) & ~(size_t)15; return o; };
  const size_t B = (size_t)h.num_games;
  if (h.kind == 0) {
    L.seeds = take(4 * B); L.key = take(4 * B); L.t = take(4 * B); L.turn = take(4 * B);
  } else {
    L.board = take(B * (size_t)h.rows * h.cols); L.player = take(B); L.lines = take(4 * (size_t)h.num_lines * h.k);
  }
  L.total = at;
  return L;
}

inline void game_device_point(GameView* v, char* base, const GameDeviceLayout& L) {
  if (v->kind == 0) {
    v->seeds = (uint32_t*)(base + L.seeds); v->key = (uint32_t*)(base + L.key); v->t = (uint32_t*)(base + L.t);
    v->turn = (int32_t*)(base + L.turn);
  } else {
    v->board = (int8_t*)(base + L.board); v->player = (int8_t*)(base + L.player); v->lines = (const int32_t*)(base + L.lines);
  }
}

// the state arrays of a view, one (pointer, bytes) pair per array that changes while games are played or restarted
template <class F>
inline void game_state_arrays(const GameView& v, F&& each) {
  const size_t B = (size_t)v.num_games;
  if (v.kind == 0) { each((void*)v.key, 4 * B); each((void*)v.t, 4 * B); each((void*)v.turn, 4 * B); }
  else { each((void*)v.board, B * (size_t)v.rows * v.cols); each((void*)v.player, B); }
}

// fn(dst array, src array, bytes) for every state array of two views of the same kind and size (host and device twin)
template <class F>
inline void game_state_copy(const GameView& dst, const GameView& src, F&& fn) {
  void* to[3];
  int n = 0, i = 0;
  game_state_arrays(dst, [&](void* p, size_t) { to[n++] = p; });
  game_state_arrays(src, [&](void* p, size_t bytes) { fn(to[i++], p, bytes); });
}

}  // namespace mzx
