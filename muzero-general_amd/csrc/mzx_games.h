// mzx_games.h -- games that step NATIVELY for a whole shard (the classes: host code, no GPU; the rules they call: both
// builds): the environments a self-play shard plays without returning to the interpreter per move (mzx_selfplay_rounds,
// mzx_actor.h).
//
// What they restate.  The reference steps one `Game` object per actor in Python (self_play.py:129-181:
// legal_actions / step / to_play per move, games/abstract_game.py:9-105).  mzx.games ships three of its board games in
// the batched plugin protocol (numpy arithmetic over [B][cells]); these are the same games -- and the synthetic
// fixed-shape environment of the metric (mzx/synthetic.py) -- behind a C ABI:
//   "synthetic"  mzx.synthetic.make_synthetic_batched_game: next observation = counter hash of (key, action, t), reward =
//                one hash bit, every action always legal, never ends before max_moves;
//   "tictactoe"  games/tictactoe.py:125-310   3 x 3, three in a row, int32 planes, a win pays 20;
//   "connect4"   games/connect4.py:125-300    6 x 7 with gravity, four in a row, float64 planes, a win pays 10;
//   "gomoku"     games/gomoku.py:130-300      11 x 11, five in a row, float64 planes, 1 is paid whenever the game ends.
// Observations are emitted as float32 (what torch.tensor(obs).float() makes of them, self_play.py:280-285; board planes
// hold -1 / 0 / 1: exact); `obs_dtype` names the dtype the reference game returns so that the host mirror hands out
// GameHistory.observation_history in it.  Game for game identical to the Python classes: tests/test_native_games.py.
//
// One source for both builds.  The per-game RULES -- the counter hash, a board cell as an observation element, the cell a
// move lands on, "this line is won", "this action is free", what an ended game pays -- are MZX_HD functions over a plain
// view of a shard's state (GameView: raw arrays, the same struct whether they are this file's vectors or device memory).
// The classes below call them in their per-game loops; the device twin (mzx_games_device.h) calls the same functions
// from one wavefront per game.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "mzx_platform.h"

namespace mzx {

struct GameView {
  int32_t kind = 0;                 // 0 synthetic, 1 k in a row
  int32_t num_games = 0, num_actions = 0, num_players = 1, obs_elems = 0;
  // synthetic: [B] each
  uint32_t* seeds = nullptr;
  uint32_t* key = nullptr;
  uint32_t* t = nullptr;
  int32_t* turn = nullptr;          // whose move it is, 0 .. num_players - 1
  // k in a row
  int32_t rows = 0, cols = 0, k = 0, gravity = 0, end_pays = 0, reward_scale = 1, num_lines = 0;
  int8_t* board = nullptr;          // [B][rows * cols]: 0 empty, 1 / -1
  int8_t* player = nullptr;         // [B]: 1 / -1
  const int32_t* lines = nullptr;   // [num_lines][k] flat cell indices
};

MZX_HD inline uint32_t game_hash_u32(uint32_t x) {     // mzx/synthetic.py _hash_u32 (wrapping 32-bit arithmetic)
  x = (x ^ 61u) ^ (x >> 16);
  x *= 9u;
  x ^= x >> 4;
  x *= 0x27D4EB2Du;
  x ^= x >> 15;
  return x;
}

// ---- synthetic (mzx/synthetic.py make_synthetic_batched_game)
// (seeds * 7919 + 17 in uint64, truncated to uint32: the same value modulo 2**32)
MZX_HD inline uint32_t synth_first_key(uint32_t seed64_low) { return game_hash_u32(seed64_low * 7919u + 17u); }
MZX_HD inline float synth_obs_elem(uint32_t key, int64_t j) {
  const uint32_t lane = (uint32_t)((uint64_t)j * 2654435761ull);
  const uint32_t h = game_hash_u32(lane + key);
  return (float)((double)h / 4294967296.0);
}
MZX_HD inline uint32_t synth_next_key(uint32_t key, int64_t action, uint32_t t_after) {
  uint32_t k = key * 31u;
  k += (uint32_t)action * 131u;
  k += t_after;
  return game_hash_u32(k);
}
MZX_HD inline int32_t synth_next_turn(int32_t turn, int32_t num_players) { return num_players > 1 ? (turn + 1) % num_players : turn; }
MZX_HD inline double synth_reward(uint32_t key) { return (double)(key & 1u); }

// ---- k in a row (mzx/games.py _KInARowBatched); b: the game's board
// element j of plane 0 / 1 / 2: my stones, the other side's, the side to move
MZX_HD inline float kin_obs_elem(int8_t cell, int8_t player, int plane) {
  return plane == 0 ? (cell == 1 ? 1.f : 0.f) : plane == 1 ? (cell == -1 ? 1.f : 0.f) : (float)player;
}
MZX_HD inline bool kin_action_free(const GameView& v, const int8_t* b, int a) {
  return v.gravity ? b[(v.rows - 1) * v.cols + a] == 0 : b[a] == 0;
}
// the cell a move lands on: the lowest empty cell of the column (-1: the reference's loop places nothing in a full one),
// or the cell itself
MZX_HD inline int kin_landing_cell(const GameView& v, const int8_t* b, int a) {
  if (!v.gravity) return a;
  for (int r = 0; r < v.rows; ++r)
    if (b[r * v.cols + a] == 0) return r * v.cols + a;
  return -1;
}
// the board with `me` on `placed` (-1: as stored) -- a wavefront judges the position before its one lane stores the stone
MZX_HD inline int8_t kin_cell(const int8_t* b, int c, int placed, int8_t me) { return c == placed ? me : b[c]; }
MZX_HD inline bool kin_line_won(const GameView& v, const int8_t* b, int l, int placed, int8_t me) {
  bool all = true;
  for (int i = 0; i < v.k && all; ++i) all = kin_cell(b, v.lines[(size_t)l * v.k + i], placed, me) == me;
  return all;
}
// element j of "can anybody still move": top cells of the columns under gravity, every cell otherwise
MZX_HD inline int kin_move_cells(const GameView& v) { return v.gravity ? v.cols : v.rows * v.cols; }
MZX_HD inline bool kin_move_cell_taken(const GameView& v, const int8_t* b, int j, int placed, int8_t me) {
  return kin_cell(b, v.gravity ? (v.rows - 1) * v.cols + j : j, placed, me) != 0;
}
MZX_HD inline double kin_reward(const GameView& v, bool won, bool over) {
  return (v.end_pays ? over : won) ? (double)v.reward_scale : 0.0;
}
MZX_HD inline int32_t kin_to_play(int8_t player) { return player == 1 ? 0 : 1; }

}  // namespace mzx

struct mzx_game {
  int32_t num_games = 0, num_actions = 0, num_players = 1;
  int32_t shape[3] = {0, 0, 0};
  int32_t obs_dtype = 0;       // 0 float32, 1 int32, 2 float64 (the reference game's array dtype)
  int32_t reward_is_int = 1;   // every shipped game pays integers
  int32_t always_all_legal = 0;
  virtual ~mzx_game() {}
  int64_t obs_elems() const { return (int64_t)shape[0] * shape[1] * shape[2]; }
  // games [lo, hi) -- every method is safe to call on disjoint ranges from several threads
  virtual void reset(const int32_t* idx, int32_t count) = 0;                  // idx == nullptr: games 0 .. count - 1
  virtual void observe(int lo, int hi, float* out) const = 0;                  // out: row g at out + g * obs_elems()
  virtual void legal_actions(int lo, int hi, int32_t* out) const = 0;          // [B][A] increasing, padded with -1
  virtual void to_play(int lo, int hi, int32_t* out) const = 0;
  // active (nullable): games with active[g] == 0 are left untouched (reward 0, not done) -- the lock-step loop of
  // SelfPlay.play_games keeps stepping a shard whose shorter games have ended
  virtual void step(int lo, int hi, const int64_t* actions, const uint8_t* active, double* reward, uint8_t* done) = 0;
  // the object's state as raw arrays (what the rules read and the device twin uploads / downloads)
  virtual mzx::GameView view() const = 0;
};

namespace mzx {

// mzx/synthetic.py make_synthetic_batched_game
struct SyntheticGame : mzx_game {
  std::vector<uint32_t> seeds, key, t;
  std::vector<int32_t> player;

  GameView view() const override {
    GameView v;
    v.kind = 0; v.num_games = num_games; v.num_actions = num_actions; v.num_players = num_players; v.obs_elems = (int32_t)obs_elems();
    v.seeds = const_cast<uint32_t*>(seeds.data()); v.key = const_cast<uint32_t*>(key.data()); v.t = const_cast<uint32_t*>(t.data());
    v.turn = const_cast<int32_t*>(player.data());
    return v;
  }
  void reset(const int32_t* idx, int32_t count) override {
    for (int32_t k = 0; k < count; ++k) {
      const int g = idx ? idx[k] : k;
      t[g] = 0; player[g] = 0;
      key[g] = synth_first_key(seeds[g]);
    }
  }
  void observe(int lo, int hi, float* out) const override {
    const int64_t E = obs_elems();
    for (int g = lo; g < hi; ++g) {
      float* o = out + (int64_t)g * E;
      for (int64_t j = 0; j < E; ++j) o[j] = synth_obs_elem(key[g], j);
    }
  }
  void legal_actions(int lo, int hi, int32_t* out) const override {
    for (int g = lo; g < hi; ++g)
      for (int a = 0; a < num_actions; ++a) out[(int64_t)g * num_actions + a] = a;
  }
  void to_play(int lo, int hi, int32_t* out) const override {
    for (int g = lo; g < hi; ++g) out[g] = player[g];
  }
  void step(int lo, int hi, const int64_t* actions, const uint8_t* /*active: the Python class steps every game*/, double* reward,
            uint8_t* done) override {
    for (int g = lo; g < hi; ++g) {
      t[g] += 1u;
      key[g] = synth_next_key(key[g], actions[g], t[g]);
      player[g] = synth_next_turn(player[g], num_players);
      reward[g] = synth_reward(key[g]);
      done[g] = 0;
    }
  }
};

// mzx/games.py _KInARowBatched
struct KInARowGame : mzx_game {
  int rows = 0, cols = 0, k = 0;
  bool gravity = false, end_pays = false;
  int reward_scale = 1;
  std::vector<int8_t> board;        // [B][rows * cols]: 0 empty, 1 / -1
  std::vector<int8_t> player;       // [B]: 1 / -1
  std::vector<int32_t> lines;       // [L][k] flat cell indices

  GameView view() const override {
    GameView v;
    v.kind = 1; v.num_games = num_games; v.num_actions = num_actions; v.num_players = num_players; v.obs_elems = (int32_t)obs_elems();
    v.rows = rows; v.cols = cols; v.k = k; v.gravity = gravity ? 1 : 0; v.end_pays = end_pays ? 1 : 0; v.reward_scale = reward_scale;
    v.num_lines = (int32_t)(lines.size() / (size_t)k);
    v.board = const_cast<int8_t*>(board.data()); v.player = const_cast<int8_t*>(player.data()); v.lines = lines.data();
    return v;
  }
  void build_lines() {
    static const int dirs[4][2] = {{0, 1}, {1, 0}, {1, 1}, {1, -1}};
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        for (const auto& d : dirs) {
          const int rr = r + (k - 1) * d[0], cc = c + (k - 1) * d[1];
          if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
          for (int i = 0; i < k; ++i) lines.push_back((r + i * d[0]) * cols + (c + i * d[1]));
        }
  }
  void reset(const int32_t* idx, int32_t count) override {
    const int cells = rows * cols;
    for (int32_t q = 0; q < count; ++q) {
      const int g = idx ? idx[q] : q;
      memset(&board[(size_t)g * cells], 0, (size_t)cells);
      player[g] = 1;
    }
  }
  void observe(int lo, int hi, float* out) const override {
    const int cells = rows * cols;
    for (int g = lo; g < hi; ++g) {
      float* o = out + (int64_t)g * 3 * cells;
      const int8_t* b = &board[(size_t)g * cells];
      for (int j = 0; j < cells; ++j)
        for (int plane = 0; plane < 3; ++plane) o[plane * cells + j] = kin_obs_elem(b[j], player[g], plane);
    }
  }
  void legal_actions(int lo, int hi, int32_t* out) const override {
    const int cells = rows * cols, A = num_actions;
    const GameView v = view();
    for (int g = lo; g < hi; ++g) {
      const int8_t* b = &board[(size_t)g * cells];
      int32_t* o = out + (int64_t)g * A;
      int n = 0;
      for (int a = 0; a < A; ++a)
        if (kin_action_free(v, b, a)) o[n++] = a;
      for (; n < A; ++n) o[n] = -1;
    }
  }
  void to_play(int lo, int hi, int32_t* out) const override {
    for (int g = lo; g < hi; ++g) out[g] = kin_to_play(player[g]);
  }
  void step(int lo, int hi, const int64_t* actions, const uint8_t* active, double* reward, uint8_t* done) override {
    const int cells = rows * cols;
    const GameView v = view();
    const int L = v.num_lines, M = kin_move_cells(v);
    for (int g = lo; g < hi; ++g) {
      if (active && !active[g]) { reward[g] = 0.0; done[g] = 0; continue; }
      int8_t* b = &board[(size_t)g * cells];
      const int a = (int)actions[g];
      const int8_t me = player[g];
      const int cell = kin_landing_cell(v, b, a);
      if (cell >= 0) b[cell] = me;
      bool won = false;
      for (int l = 0; l < L && !won; ++l) won = kin_line_won(v, b, l, -1, me);
      bool no_move = true;
      for (int j = 0; j < M && no_move; ++j) no_move = kin_move_cell_taken(v, b, j, -1, me);
      const bool over = won || no_move;
      done[g] = over ? 1 : 0;
      reward[g] = kin_reward(v, won, over);
      player[g] = (int8_t)-me;
    }
  }
};

// kind, geometry -> a game object (nullptr + message on a bad argument)
inline mzx_game* game_make(const char* kind, int32_t num_games, const uint32_t* seeds, const int32_t shape[3], int32_t num_actions,
                           int32_t num_players, std::string& err) {
  if (!kind || num_games < 1) { err = "mzx_game_create: kind / num_games"; return nullptr; }
  const std::string name(kind);
  if (name == "synthetic") {
    if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || num_actions < 1 || num_players < 1) {
      err = "mzx_game_create(synthetic): observation shape, actions and players must be positive";
      return nullptr;
    }
    SyntheticGame* g = new SyntheticGame();
    g->num_games = num_games; g->num_actions = num_actions; g->num_players = num_players;
    g->shape[0] = shape[0]; g->shape[1] = shape[1]; g->shape[2] = shape[2];
    g->obs_dtype = 0; g->always_all_legal = 1;
    g->seeds.resize(num_games); g->key.resize(num_games); g->t.assign(num_games, 0); g->player.assign(num_games, 0);
    for (int i = 0; i < num_games; ++i) g->seeds[i] = seeds ? seeds[i] : 0u;
    g->reset(nullptr, num_games);
    return g;
  }
  KInARowGame* g = nullptr;
  if (name == "tictactoe") { g = new KInARowGame(); g->rows = 3; g->cols = 3; g->k = 3; g->reward_scale = 20; g->obs_dtype = 1; }
  else if (name == "connect4") { g = new KInARowGame(); g->rows = 6; g->cols = 7; g->k = 4; g->gravity = true; g->reward_scale = 10; g->obs_dtype = 2; }
  else if (name == "gomoku") { g = new KInARowGame(); g->rows = 11; g->cols = 11; g->k = 5; g->reward_scale = 1; g->obs_dtype = 2; g->end_pays = true; }
  else { err = "mzx_game_create: unknown game '" + name + "' (synthetic, tictactoe, connect4, gomoku)"; return nullptr; }
  g->num_games = num_games; g->num_players = 2;
  g->num_actions = g->gravity ? g->cols : g->rows * g->cols;
  g->shape[0] = 3; g->shape[1] = g->rows; g->shape[2] = g->cols;
  g->board.assign((size_t)num_games * g->rows * g->cols, 0);
  g->player.assign(num_games, 1);
  g->build_lines();
  return g;
}

}  // namespace mzx
