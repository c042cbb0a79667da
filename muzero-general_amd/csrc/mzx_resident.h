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
//
// Here: the device state and the wave bodies (vote, commit, gather), then the host side of a group: the layout of its block,
// a round queued (resident_queue_round), the chunk's downloads and harvest, the repair of a halted round and the loop of a
// call (resident_rounds).  mzx_actor_set_resident and mzx_selfplay_rounds (mzx_lib.cpp) check arguments and call in here.
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

// The hand-off's gather (mzx_actor_set_device_handoff): the same packed arrays, one wavefront per packed ROW -- work item e
// is row e of the (len + 1)-long arrays and finds its game by binary search over the table's offset column, as
// ReplayIngestRowBody (mzx_replay.h) does; no game's moves are walked one after another.  Row 0 of a game also writes the
// game's entries of the three columns mzx_replay_ingest reads straight from the device: len i32, src1 / src0 i64.
struct ResidentPackBody {
  ResidentDevice d;
  const int64_t* table;                // [count][5] as the gather's; column 3 strictly increasing from 0
  int32_t count, q_first;
  int64_t r_first, total_rows;         // total_rows = sum(len + 1)
  float* obs; int64_t* act; int64_t* tp; double* rew; int32_t* vis; double* val; uint8_t* mask;
  int32_t* len; int64_t* src1; int64_t* src0;
  MZX_HD size_t size() const { return (size_t)total_rows; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int64_t r = (int64_t)e;
    int lo = 0, hi = count - 1;        // table[lo][3] <= r always; the same search in every lane
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (table[5 * (size_t)mid + 3] <= r) lo = mid; else hi = mid - 1;
    }
    const int64_t* t = table + 5 * (size_t)lo;
    const int64_t st = t[0], s = t[1], n = t[2], q1 = t[3], q0 = t[4];
    const int64_t m = r - q1;
    if (m < 0 || m > n) return;
    const int A = d.A, E = d.E, B = d.B;
    if (m < n) {
      const size_t row = (size_t)((st + m) % d.cap) * B + (size_t)s;
      WAVE_FOR(j, E) obs[(size_t)r * E + j] = d.l_obs[row * E + j];
      WAVE_FOR(j, A) vis[(size_t)(q0 + m) * A + j] = d.l_vis[row * A + j];
      if (mask) WAVE_FOR(j, A) mask[(size_t)(q0 + m) * A + j] = d.l_mask[row * A + j];
      if (lane == 0) {
        tp[r] = d.l_tp[row];
        act[r + 1] = d.l_act[row];
        rew[r + 1] = d.l_rew[row];
        val[q0 + m] = d.l_val[row];
      }
    } else {                           // the position after the last move closes the record
      const size_t cell = (size_t)((st + n - 1 - r_first) + q_first) * B + (size_t)s;
      WAVE_FOR(j, E) obs[(size_t)r * E + j] = d.fin_obs[cell * E + j];
      if (lane == 0) tp[r] = d.fin_tp[cell];
    }
    if (m == 0 && lane == 0) {
      act[q1] = 0; rew[q1] = 0.0;      // action_history / reward_history start with 0 (self_play.py:118-120)
      len[lo] = (int32_t)n; src1[lo] = q1; src0[lo] = q0;
    }
  }
};

}  // namespace mzx

// A piece: the finished games one harvest of a hand-off group packed, kept ON THE DEVICE in a buffer the actor owns -- the
// packed arrays in the staged layout of mzx_replay_ingest and the len / src1 / src0 columns -- with the per-game slot /
// length / sequence on the host.  free -> (harvest) queued -> (mzx_actor_take_device) taken -> (mzx_actor_release_device)
// free again once the event recorded at the release has passed.
struct mzx_actor_piece {
  enum State { FREE, FILLING, QUEUED, TAKEN };
  int64_t token = 0;
  void* buf = nullptr;
  int64_t bytes = 0;
  State state = FREE;
  void* event = nullptr;               // recorded by the release behind the consumer's work
  bool event_pending = false;
  int64_t games = 0, rows0 = 0;        // rows0 = sum len
  bool mask = false;
  size_t o_len = 0, o_src1 = 0, o_src0 = 0, o_obs = 0, o_act = 0, o_tp = 0, o_rew = 0, o_vis = 0, o_val = 0, o_mask = 0;
  std::vector<int32_t> slot, n;
  std::vector<int64_t> seq;
};

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
  // the device hand-off (mzx_actor_set_device_handoff); pieces / queued / piece_bytes under the actor's finished_lock
  bool handoff = false;
  int64_t max_log_bytes = 0, next_token = 1, piece_bytes = 0;
  std::vector<std::unique_ptr<mzx_actor_piece>> pieces;
  std::deque<mzx_actor_piece*> queued;
};

namespace mzx {

// ---- the group's device block ------------------------------------------------------------------------------------------

// byte offsets of the arrays of a group (sizes of `d` set) inside its one block, each 16-byte aligned; total: the block's size
struct ResidentLayout { size_t start, temps, obs, tp, act, vis, val, rew, mask, ctrl, fin_tp, fin_obs, total; };
inline ResidentLayout resident_layout(const ResidentDevice& d) {
  const size_t B = (size_t)d.B, A = (size_t)d.A, E = (size_t)d.E, rows = (size_t)d.cap * B, cells = (size_t)d.chunk * B;
  ResidentLayout L;
  Carver c;
  L.start = c.take(8 * B); L.temps = c.take(8 * B); L.obs = c.take(4 * rows * E); L.tp = c.take(4 * rows); L.act = c.take(8 * rows);
  L.vis = c.take(4 * rows * A); L.val = c.take(8 * rows); L.rew = c.take(8 * rows); L.mask = c.take(d.masks ? rows * A : 0);
  L.ctrl = c.take(4 * (RESIDENT_CTRL_WORDS + cells)); L.fin_tp = c.take(4 * cells); L.fin_obs = c.take(4 * cells * E);
  L.total = c.at;
  return L;
}

inline void resident_point(ResidentDevice* d, char* base, const ResidentLayout& L) {
  d->start = (int64_t*)(base + L.start); d->temps = (double*)(base + L.temps); d->l_obs = (float*)(base + L.obs);
  d->l_tp = (int32_t*)(base + L.tp); d->l_act = (int64_t*)(base + L.act); d->l_vis = (int32_t*)(base + L.vis);
  d->l_val = (double*)(base + L.val); d->l_rew = (double*)(base + L.rew); d->l_mask = d->masks ? (uint8_t*)(base + L.mask) : nullptr;
  d->ctrl = (int32_t*)(base + L.ctrl); d->fin_len = d->ctrl + RESIDENT_CTRL_WORDS; d->fin_tp = (int32_t*)(base + L.fin_tp);
  d->fin_obs = (float*)(base + L.fin_obs);
}

inline void resident_free(mzx_actor* a) {
  mzx_actor_resident* R = a->resident;
  if (!R) return;
  mzx_game_device_destroy(R->game);
  if (R->block) device_free(R->block);
  if (R->d_pack) device_free(R->d_pack);
  if (!R->pieces.empty()) device_sync();        // (a consumer's launch may still be reading a piece)
  for (auto& p : R->pieces) {
    event_destroy(p->event);
    if (p->buf) device_free(p->buf);
  }
  delete R;
  a->resident = nullptr;
}

// ---- the pieces of a hand-off group ---------------------------------------------------------------------------------------

inline void resident_piece_drop(mzx_actor_resident* R, size_t index) {
  mzx_actor_piece* p = R->pieces[index].get();
  event_destroy(p->event);
  if (p->buf) device_free(p->buf);
  R->piece_bytes -= p->bytes;
  R->stats[7] = R->piece_bytes;
  R->pieces.erase(R->pieces.begin() + (long)index);
}

// A buffer of at least `need` bytes for the next piece: a free one whose release event has passed (a pending event is
// queried, never waited for), else a fresh allocation.  Device log plus pieces stay within the group's max_log_bytes: free
// buffers that are too small are given back first, and what still does not fit is refused with the sizes.
inline int resident_piece_acquire(mzx_actor* a, size_t need, mzx_actor_piece** out) {
  mzx_actor_resident* R = a->resident;
  std::lock_guard<std::mutex> lk(a->finished_lock);
  for (auto& p : R->pieces)
    if (p->state == mzx_actor_piece::FREE && (size_t)p->bytes >= need && (!p->event_pending || event_done(p->event))) {
      p->event_pending = false;
      p->state = mzx_actor_piece::FILLING;
      *out = p.get();
      return MZX_OK;
    }
  size_t want = std::max(need, (size_t)1 << 16) * 2;
  if (R->block_bytes + R->piece_bytes + (int64_t)want > R->max_log_bytes) {
    for (size_t i = R->pieces.size(); i-- > 0;) {
      mzx_actor_piece* p = R->pieces[i].get();
      if (p->state == mzx_actor_piece::FREE && (!p->event_pending || event_done(p->event))) resident_piece_drop(R, i);
    }
    want = (need + 15) / 16 * 16;
  }
  if (R->block_bytes + R->piece_bytes + (int64_t)want > R->max_log_bytes) {
    set_error("mzx_selfplay_rounds (resident): the device log (%lld bytes) and the pieces kept on the device (%lld bytes) leave no room "
              "for a piece of %lld bytes within max_log_bytes = %lld: release pieces (mzx_actor_release_device) or raise the bound",
              (long long)R->block_bytes, (long long)R->piece_bytes, (long long)want, (long long)R->max_log_bytes);
    return MZX_ERR_INVALID;
  }
  std::unique_ptr<mzx_actor_piece> p(new (std::nothrow) mzx_actor_piece());
  if (!p) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  if (device_alloc(&p->buf, want) != 0) { set_error("mzx_selfplay_rounds (resident): piece buffer of %lld bytes", (long long)want); return MZX_ERR_RUNTIME; }
  p->bytes = (int64_t)want;
  p->state = mzx_actor_piece::FILLING;
  R->piece_bytes += p->bytes;
  R->stats[7] = R->piece_bytes;
  *out = p.get();
  R->pieces.push_back(std::move(p));
  return MZX_OK;
}

inline mzx_actor_piece* resident_piece_find(mzx_actor_resident* R, int64_t token, mzx_actor_piece::State state) {
  for (auto& p : R->pieces)
    if (p->token == token && p->state == state) return p.get();
  return nullptr;
}

// ---- the rounds of a call (mzx_selfplay_rounds with resident groups) -----------------------------------------------------

constexpr int32_t RESIDENT_CTRL_CLEAR[RESIDENT_CTRL_WORDS] = {0, -1, 0, 0};

struct ResidentPiece {            // the games one harvest of one group brought, not yet numbered
  int group;
  mzx_actor::Batch b;             // (a hand-off group: slot / n / seq only -- the arrays stay on the device, in `device`)
  mzx_actor_piece* device = nullptr;
  std::vector<int64_t> round;     // round of the CALL each game ended in
};

inline int resident_fail(const char* what, int rc) {
  set_error("mzx_selfplay_rounds (resident): %s: %s", what, runtime_error_string(rc));
  return MZX_ERR_RUNTIME;
}

// draws -> search -> action choice of the group's next position under `counter`
inline int resident_queue_search(mzx_actor* a, const RoundsArgs& args, uint64_t counter, void* stream) {
  mzx_draws d; mzx_draws_select sel;
  actor_draws(a, args, counter, &d, &sel);
  return actor_queue_device_move(a->search, &a->move, &d, &sel, a->d_arena, a->arena_bytes, stream);
}

inline int resident_queue_commit(mzx_actor* a, const RoundsArgs& args, int64_t r, int q, int prime, void* stream) {
  ResidentCommitBody body{a->resident->d, r, q, prime, args.temperature_threshold, args.temperature};
  const int rc = launch_waves<GAME_WAVES>(body, (stream_t)stream);
  return rc ? resident_fail("commit launch", rc) : MZX_OK;
}

// round r of the group as round q of the chunk, searched under `counter`: search -> vote -> commit, nothing waited for
inline int resident_queue_round(mzx_actor* a, const RoundsArgs& args, int q, int64_t r, uint64_t counter, void* stream) {
  int rc = resident_queue_search(a, args, counter, stream);
  if (rc) return rc;
  rc = launch_waves<GAME_WAVES>(ResidentVoteBody{a->resident->d, q}, (stream_t)stream);
  if (rc) return resident_fail("vote launch", rc);
  return resident_queue_commit(a, args, r, q, 0, stream);
}

// rounds [q0, q1) of the chunk for one group, the first one round a->round under a->draw_counter (the rest of a chunk behind a
// repaired round)
inline int resident_queue_rounds(mzx_actor* a, const RoundsArgs& args, int q0, int q1, void* stream) {
  int rc = MZX_OK;
  for (int q = q0; q < q1 && rc == MZX_OK; ++q)
    rc = resident_queue_round(a, args, q, a->round + (q - q0), a->draw_counter + (uint64_t)(q - q0), stream);
  return rc;
}

// the downloads of a chunk's end: control block + finished lengths, and the game state into the host game object (so that
// legal_actions() etc. are true between calls); queued behind the chunk's rounds, waited for by resident_wait
inline int resident_queue_downloads(mzx_actor* a, int rounds_of_chunk, void* stream) {
  mzx_actor_resident* R = a->resident;
  const size_t bytes = sizeof(int32_t) * (RESIDENT_CTRL_WORDS + (size_t)rounds_of_chunk * a->B);
  int rc = copy_d2h(R->h_ctrl.data(), R->d.ctrl, bytes, (stream_t)stream);
  if (rc) return resident_fail("control block download", rc);
  R->stats[4] += (int64_t)bytes;
  game_state_copy(a->game->view(), R->game->v, [&](void* to, void* from, size_t n) {
    if (rc == 0) { rc = copy_d2h(to, from, n, (stream_t)stream); R->stats[4] += (int64_t)n; }
  });
  return rc ? resident_fail("game state download", rc) : MZX_OK;
}

inline int resident_wait(mzx_actor* a, void* stream) {
  const int rc = stream_sync((stream_t)stream);
  a->resident->stats[3] += 1;
  return rc ? resident_fail("waiting for the group's stream", rc) : MZX_OK;
}

// the games that ended in rounds [q0, q1) of the chunk (round q = round r_first + (q - q0) of the group, call_round0 + q of the
// call): gathered on the device, downloaded, queued as one piece
inline int resident_harvest(mzx_actor* a, int group, int q0, int q1, int64_t r_first, int64_t call_round0, void* stream,
                            std::vector<ResidentPiece>& pieces) {
  mzx_actor_resident* R = a->resident;
  const int64_t B = a->B, A = a->A, E = a->E;
  const int32_t* fin = R->h_ctrl.data() + RESIDENT_CTRL_WORDS;
  std::vector<int64_t> table;
  ResidentPiece piece;
  piece.group = group;
  mzx_actor::Batch& b = piece.b;
  int64_t o1 = 0, o0 = 0;
  for (int q = q0; q < q1; ++q)
    for (int64_t s = 0; s < B; ++s) {
      const int64_t n = fin[(size_t)q * B + s];
      if (n == 0) continue;
      const int64_t last = r_first + (q - q0);
      if (n < 1 || n > a->max_moves || n > last + 1) {
        set_error("mzx_selfplay_rounds (resident): slot %lld reports a game of %lld moves in round %lld", (long long)s, (long long)n, (long long)last);
        return MZX_ERR_RUNTIME;
      }
      const int64_t row[5] = {last - n + 1, s, n, o1, o0};
      table.insert(table.end(), row, row + 5);
      b.slot.push_back(a->first_slot + (int32_t)s); b.n.push_back((int32_t)n); b.seq.push_back(0);
      piece.round.push_back(call_round0 + q);
      o1 += n + 1; o0 += n;
    }
  const int64_t k = (int64_t)b.slot.size();
  if (k == 0) return MZX_OK;
  const bool masks = R->d.masks != 0;
  if (R->handoff) {
    // the pack into a piece: nothing of it is downloaded; the launch has completed when this returns
    Carver c;
    mzx_actor_piece L;
    const size_t o_table = c.take(8 * table.size());
    L.o_len = c.take(4 * (size_t)k); L.o_src1 = c.take(8 * (size_t)k); L.o_src0 = c.take(8 * (size_t)k);
    L.o_obs = c.take(4 * (size_t)(o1 * E)); L.o_act = c.take(8 * (size_t)o1); L.o_tp = c.take(8 * (size_t)o1);
    L.o_rew = c.take(8 * (size_t)o1); L.o_vis = c.take(4 * (size_t)(o0 * A)); L.o_val = c.take(8 * (size_t)o0);
    L.o_mask = c.take(masks ? (size_t)(o0 * A) : 0);
    mzx_actor_piece* p = nullptr;
    int rc = resident_piece_acquire(a, c.at, &p);
    if (rc) return rc;
    p->games = k; p->rows0 = o0; p->mask = masks;
    p->o_len = L.o_len; p->o_src1 = L.o_src1; p->o_src0 = L.o_src0; p->o_obs = L.o_obs; p->o_act = L.o_act; p->o_tp = L.o_tp;
    p->o_rew = L.o_rew; p->o_vis = L.o_vis; p->o_val = L.o_val; p->o_mask = L.o_mask;
    char* base = (char*)p->buf;
    rc = copy_h2d(base + o_table, table.data(), 8 * table.size(), (stream_t)stream);
    if (rc == 0) {
      ResidentPackBody body{R->d, (const int64_t*)(base + o_table), (int32_t)k, q0, r_first, o1, (float*)(base + p->o_obs),
                            (int64_t*)(base + p->o_act), (int64_t*)(base + p->o_tp), (double*)(base + p->o_rew), (int32_t*)(base + p->o_vis),
                            (double*)(base + p->o_val), masks ? (uint8_t*)(base + p->o_mask) : nullptr, (int32_t*)(base + p->o_len),
                            (int64_t*)(base + p->o_src1), (int64_t*)(base + p->o_src0)};
      rc = launch_waves<GAME_WAVES>(body, (stream_t)stream);
    }
    const int waited = rc ? rc : resident_wait(a, stream);      // (the table is a local: it must outlive its upload)
    if (rc || waited) {
      if (rc) (void)stream_sync((stream_t)stream);
      std::lock_guard<std::mutex> lk(a->finished_lock);
      p->state = mzx_actor_piece::FREE;
      return rc ? resident_fail("pack upload / launch", rc) : waited;
    }
    piece.device = p;
    R->stats[6] += k;
    pieces.push_back(std::move(piece));
    return MZX_OK;
  }
  Carver c;
  const size_t o_table = c.take(8 * table.size()), o_obs = c.take(4 * (size_t)(o1 * E)), o_act = c.take(8 * (size_t)o1), o_tp = c.take(8 * (size_t)o1),
               o_rew = c.take(8 * (size_t)o1), o_vis = c.take(4 * (size_t)(o0 * A)), o_val = c.take(8 * (size_t)o0), o_mask = c.take(masks ? (size_t)(o0 * A) : 0);
  if ((int64_t)c.at > R->pack_bytes) {
    if (R->d_pack) device_free(R->d_pack);
    R->d_pack = nullptr; R->pack_bytes = 0;
    const size_t want = std::max(c.at, (size_t)1 << 16) * 2;
    if (device_alloc(&R->d_pack, want) != 0) { R->d_pack = nullptr; set_error("mzx_selfplay_rounds (resident): gather buffer of %lld bytes", (long long)want); return MZX_ERR_RUNTIME; }
    R->pack_bytes = (int64_t)want;
  }
  char* base = (char*)R->d_pack;
  int rc = copy_h2d(base + o_table, table.data(), 8 * table.size(), (stream_t)stream);
  if (rc) return resident_fail("gather table upload", rc);
  ResidentGatherBody body{R->d, (const int64_t*)(base + o_table), (int32_t)k, q0, r_first, (float*)(base + o_obs), (int64_t*)(base + o_act),
                          (int64_t*)(base + o_tp), (double*)(base + o_rew), (int32_t*)(base + o_vis), (double*)(base + o_val),
                          masks ? (uint8_t*)(base + o_mask) : nullptr};
  rc = launch_waves<GAME_WAVES>(body, (stream_t)stream);
  if (rc) return resident_fail("gather launch", rc);
  b.obs.resize((size_t)(o1 * E)); b.act.resize((size_t)o1); b.tp.resize((size_t)o1); b.rew.resize((size_t)o1);
  b.vis.resize((size_t)(o0 * A)); b.val.resize((size_t)o0);
  if (masks) b.mask.resize((size_t)(o0 * A));
  struct { void* dst; const void* src; size_t bytes; } copies[7] = {
      {b.obs.data(), base + o_obs, 4 * b.obs.size()}, {b.act.data(), base + o_act, 8 * b.act.size()}, {b.tp.data(), base + o_tp, 8 * b.tp.size()},
      {b.rew.data(), base + o_rew, 8 * b.rew.size()}, {b.vis.data(), base + o_vis, 4 * b.vis.size()}, {b.val.data(), base + o_val, 8 * b.val.size()},
      {b.mask.data(), base + o_mask, b.mask.size()}};
  for (const auto& cp : copies) {
    if (cp.bytes == 0) continue;
    rc = copy_d2h(cp.dst, cp.src, cp.bytes, (stream_t)stream);
    if (rc) return resident_fail("finished games download", rc);
    R->stats[4] += (int64_t)cp.bytes;
  }
  rc = resident_wait(a, stream);
  if (rc) return rc;
  if (masks) {
    bool any_illegal = false;
    for (uint8_t x : b.mask) if (!x) { any_illegal = true; break; }
    if (!any_illegal) { b.mask.clear(); b.mask.shrink_to_fit(); }
  }
  R->stats[6] += k;
  pieces.push_back(std::move(piece));
  return MZX_OK;
}

// the rare path: round a->round halted (a tree exhausted its tie-break tape).  The round is searched again under the same
// counter and waited for, the flagged trees go through actor_retry_flagged on the host mirrors of the move's blocks (as
// actor_consume's do on its vectors), the patched output block goes back and the round is committed.
inline int resident_repair(mzx_actor* a, int group, const RoundsArgs& args, int q, void* stream) {
  mzx_actor_resident* R = a->resident;
  const mzx_move* m = &a->move;
  const uint64_t counter = a->draw_counter;
  int rc = resident_queue_search(a, args, counter, stream);
  if (rc) return rc;
  if (m->h_in != m->d_in) { rc = copy_d2h(m->h_in, m->d_in, (size_t)m->in_bytes, (stream_t)stream); R->stats[4] += m->in_bytes; }
  if (rc == 0 && m->h_out != m->d_out) { rc = copy_d2h(m->h_out, m->d_out, (size_t)m->out_bytes, (stream_t)stream); R->stats[4] += m->out_bytes; }
  if (rc) return resident_fail("download of the halted round", rc);
  rc = resident_wait(a, stream);
  if (rc) return rc;
  a->draw_counter = counter + 1;        // (the retry callback reads mzx_actor_draw_counter - 1)
  std::vector<int32_t> redo;
  rc = actor_retry_flagged(a, group, args, move_out_host(m, m->io.d_info), counter,
                           ActorRows{move_in_host(m, m->io.d_legal_actions), move_out_host(m, m->io.d_visit_counts),
                                     move_in_host(m, a->d_temperature), move_out_host(m, a->d_action)}, &redo);
  if (rc) return rc;
  if (m->h_out != m->d_out) {
    rc = copy_h2d(m->d_out, m->h_out, (size_t)m->out_bytes, (stream_t)stream);
    if (rc) return resident_fail("upload of the repaired round", rc);
  }
  rc = copy_h2d(R->d.ctrl, RESIDENT_CTRL_CLEAR, sizeof(RESIDENT_CTRL_CLEAR), (stream_t)stream);
  if (rc) return resident_fail("control block reset", rc);
  rc = resident_queue_commit(a, args, a->round, q, 0, stream);
  if (rc) return rc;
  a->round += 1;
  R->stats[0] += 1; R->stats[2] += 1;
  return MZX_OK;
}

inline int resident_rounds(mzx_actor* const* groups, int num_groups, mzx_rounds* io, const RoundsArgs& args, const std::vector<void*>& streams,
                           int64_t* out_finished, int64_t* out_rounds, int64_t* out_searches, int64_t* sequence) {
  int rc = MZX_OK;
  double* phase = io->phase_seconds;
  int chunk = groups[0]->resident->d.chunk;
  for (int k = 0; k < num_groups; ++k) chunk = std::min(chunk, (int)groups[k]->resident->d.chunk);
  for (int k = 0; k < num_groups && rc == MZX_OK; ++k) {      // the first search's inputs, written by the device from the games' state
    mzx_actor* a = groups[k];
    mzx_actor_resident* R = a->resident;
    if (R->primed) continue;
    const double t0 = actor_now();
    void* st = streams[(size_t)k];
    if ((rc = copy_h2d(R->d.start, a->start.data(), 8 * (size_t)a->B, (stream_t)st)) != 0 ||
        (rc = copy_h2d(R->d.temps, a->temps.data(), 8 * (size_t)a->B, (stream_t)st)) != 0 ||
        (rc = copy_h2d(R->d.ctrl, RESIDENT_CTRL_CLEAR, sizeof(RESIDENT_CTRL_CLEAR), (stream_t)st)) != 0) {
      rc = resident_fail("first upload", rc);
      break;
    }
    rc = resident_queue_commit(a, args, a->round, 0, 1, st);
    R->primed = rc == MZX_OK;
    phase[0] += actor_now() - t0;
  }
  int64_t finished = 0, rounds = 0, searches = 0;
  while (rc == MZX_OK && finished < io->min_games && (io->max_rounds < 0 || rounds < io->max_rounds)) {
    const int n = io->max_rounds < 0 ? chunk : (int)std::min<int64_t>(chunk, io->max_rounds - rounds);
    std::vector<ResidentPiece> pieces;
    double t0 = actor_now();
    // the chunk's rounds, interleaved round by round so that every group's stream starts at once
    for (int q = 0; q < n && rc == MZX_OK; ++q)
      for (int k = 0; k < num_groups && rc == MZX_OK; ++k)
        rc = resident_queue_round(groups[k], args, q, groups[k]->round + q, groups[k]->draw_counter + (uint64_t)q, streams[(size_t)k]);
    for (int k = 0; k < num_groups && rc == MZX_OK; ++k) rc = resident_queue_downloads(groups[k], n, streams[(size_t)k]);
    phase[0] += actor_now() - t0;
    for (int k = 0; k < num_groups && rc == MZX_OK; ++k) {
      mzx_actor* a = groups[k];
      mzx_actor_resident* R = a->resident;
      void* st = streams[(size_t)k];
      // rounds of the chunk: [0, accounted) are committed and counted in a->round / a->draw_counter (a repaired round is,
      // the moment resident_repair commits it), [0, harvested) have handed out their finished games
      int accounted = 0, harvested = 0;
      R->stats[1] += 1;
      while (rc == MZX_OK) {
        t0 = actor_now();
        rc = resident_wait(a, st);
        phase[1] += actor_now() - t0;
        if (rc) break;
        const bool halted = R->h_ctrl[0] != 0;
        const int upto = halted ? R->h_ctrl[1] : n;       // the device committed rounds [accounted, upto) in this pass
        if (upto < accounted || upto > n || (halted && upto >= n)) {
          set_error("mzx_selfplay_rounds (resident): halt round %d outside the chunk's queued rounds [%d, %d)", upto, accounted, n);
          rc = MZX_ERR_RUNTIME;
          break;
        }
        t0 = actor_now();
        rc = resident_harvest(a, k, harvested, upto, a->round - (accounted - harvested), rounds, st, pieces);
        a->round += upto - accounted; a->draw_counter += (uint64_t)(upto - accounted); R->stats[0] += upto - accounted;
        accounted = harvested = upto;
        phase[3] += actor_now() - t0;
        if (rc || !halted) break;
        t0 = actor_now();
        rc = resident_repair(a, k, args, upto, st);       // (commits round `upto`: harvested with the next pass)
        accounted = upto + 1;
        if (rc == MZX_OK) rc = resident_queue_rounds(a, args, accounted, n, st);
        if (rc == MZX_OK) rc = resident_queue_downloads(a, n, st);
        phase[4] += actor_now() - t0;
      }
    }
    if (rc) {                 // (the pieces packed so far are not handed out: their buffers are free again)
      for (ResidentPiece& p : pieces)
        if (p.device) { std::lock_guard<std::mutex> lk(groups[p.group]->finished_lock); p.device->state = mzx_actor_piece::FREE; }
      break;
    }
    // sequence numbers in (round, group, slot) order across groups: the order the host loop finishes games in
    struct Key { int64_t round; int group; int32_t slot; size_t piece, j; };
    std::vector<Key> keys;
    for (size_t p = 0; p < pieces.size(); ++p)
      for (size_t j = 0; j < pieces[p].b.slot.size(); ++j) keys.push_back({pieces[p].round[j], pieces[p].group, pieces[p].b.slot[j], p, j});
    std::sort(keys.begin(), keys.end(), [](const Key& x, const Key& y) {
      return x.round != y.round ? x.round < y.round : x.group != y.group ? x.group < y.group : x.slot < y.slot;
    });
    for (const Key& key : keys) pieces[key.piece].b.seq[key.j] = (*sequence)++;
    for (ResidentPiece& p : pieces) {
      mzx_actor* a = groups[p.group];
      std::lock_guard<std::mutex> lk(a->finished_lock);
      if (p.device) {
        p.device->slot.swap(p.b.slot); p.device->n.swap(p.b.n); p.device->seq.swap(p.b.seq);
        p.device->token = a->resident->next_token++;
        p.device->state = mzx_actor_piece::QUEUED;
        a->resident->queued.push_back(p.device);
      } else {
        a->finished.push_back(std::move(p.b));
      }
    }
    finished += (int64_t)keys.size();
    rounds += n;
    for (int k = 0; k < num_groups; ++k) searches += (int64_t)n * groups[k]->B;
  }
  *out_finished = finished; *out_rounds = rounds; *out_searches = searches;
  return rc;
}

}  // namespace mzx
