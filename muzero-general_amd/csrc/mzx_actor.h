// mzx_actor.h -- the self-play ROUND LOOP of a shard of natively stepped games (host code; one call plays many moves).
//
// Reference: SelfPlay.play_game, /root/reference/self_play.py:110-183 -- per move: stacked observation, MCTS.run,
// select_action (:222-245, temperature_threshold gate :151-157), Game.step, GameHistory appends (:159-177), until done or
// max_moves (:129) -- and the actor loop around it (:31-52: the next game starts the moment one ends).  mzx.self_play
// plays B such actors as one shard (SelfPlay.play_rounds: every slot is one actor with its own numpy stream, finished
// games hand their slot to the next one, every search runs at full width); through a Python plugin game that is ~75
// interpreter statements per slot group and round around two library calls.  For a game that steps natively (mzx_games.h)
// the whole loop runs here: per round and slot group
//     begin    legal_actions / to_play / observation of the group's games -> mzx_selfplay_search (root noise + tie words
//              straight into the pinned staging block, ONE upload, the search, ONE download, not waited for)
//     consume  wait for that search's event; tape-overflow retries (callback); mzx_selfplay_select (the streams consume
//              the search's tie words, every game's action is drawn); the move is logged as one row per field of a ring
//              [round % capacity][slot]; Game.step; games that ended (done, or max_moves moves) are copied out of the ring
//              into the finished queue, their slots restart (Game.reset on the slot, same stream)
// and two slot groups take turns on the GPU exactly as SelfPlay._rounds_batched schedules them (the search of one group
// is in flight while the host consumes the other; a search is only queued ahead when the call cannot end before it is
// consumed, so nothing is in flight between calls -- weights may change there).  Same draws in the same order, same
// games field for field as the Python loop: tests/test_native_rounds.py.
//
// Resident rounds (mzx_actor_set_resident; mzx_resident.h, mzx_games_device.h): on device draws nothing of a move needs the
// host, and a group may keep its games, this log and its per-slot bookkeeping on the device -- whole rounds are queued back
// to back and the host returns once per chunk of rounds for the finished games.  The loop above is then the comparator
// (tests/resident_rounds_cases.py) and the repair path's model (tape retries).
//
// Here: the group object, actor_begin / actor_consume / actor_rounds (the host loop), and what both loops share: actor_draws,
// actor_queue_device_move (draws -> search -> action choice) and actor_retry_flagged (the tape repair).  The staging of a
// move is mzx_selfplay.h's, the resident driver mzx_resident.h's; mzx_selfplay_rounds (mzx_lib.cpp) checks and dispatches.
//
// Not here (the Python loop keeps them): stacked observations (the device frame store), Python plugin games, opponents.
#pragma once
#include <chrono>
#include <deque>
#include <memory>
#include <mutex>
#include <vector>

#include "mzx_games.h"
#include "mzx_selfplay.h"

struct mzx_actor_resident;

struct mzx_actor {
  mzx_game* game = nullptr;
  mzx_search* search = nullptr;
  mzx_rng* bank = nullptr;
  void* d_arena = nullptr;
  int64_t arena_bytes = 0;
  mzx_move move{};                       // staging blocks + io; the host-array fields point into this object's vectors
  int32_t B = 0, A = 0, max_moves = 0;
  int64_t E = 0;                         // observation elements per game
  int32_t first_slot = 0;                // slot of game 0 in the shard (finished games report shard slots)
  std::vector<int32_t> streams, legal, to_play, n_legal, words;
  std::vector<float> cur_obs, next_obs;
  std::vector<int64_t> actions, start;
  std::vector<double> temps, move_temps, reward;
  std::vector<uint8_t> done;
  int64_t round = 0;
  bool pending = false;
  void* event = nullptr;                 // recorded behind the queued download of the search in flight
  void* own_stream = nullptr;            // groups behind the first search on a stream of their own (created on first use)
  void* start_event = nullptr;           // orders that stream behind what the caller queued before the call
  // the log of the games in progress: ring rows [round % cap][slot]
  int64_t cap = 0;
  std::vector<float> r_obs;
  std::vector<int32_t> r_tp, r_vis;
  std::vector<int64_t> r_act;
  std::vector<double> r_rew, r_val;
  std::vector<uint8_t> r_mask;           // [cap][B][A], only for games whose legal sets vary
  // finished games, batch by batch (the games one consume() ended), game-major ragged arrays
  struct Batch {
    std::vector<int32_t> slot, n;
    std::vector<int64_t> seq;
    std::vector<float> obs;              // sum(n + 1) x E
    std::vector<int64_t> act, tp;        // sum(n + 1)
    std::vector<double> rew;             // sum(n + 1)
    std::vector<int32_t> vis;            // sum(n) x A
    std::vector<double> val;             // sum(n)
    std::vector<uint8_t> mask;           // sum(n) x A, empty when every action was legal throughout
  };
  // (taken by mzx_actor_take, possibly from another thread while a rounds call is appending: the queue has its own lock)
  std::deque<Batch> finished;
  std::mutex finished_lock;
  // device draws (mzx_actor_set_device_draws; mzx_draws.h): the group's search number is the counter, its slots the streams
  bool device_draws = false;
  uint64_t draw_seed = 0, draw_counter = 0;          // draw_counter: of the NEXT search
  double* d_temperature = nullptr;                    // [B] inside move.d_in
  int64_t* d_action = nullptr;                        // [B] inside move.d_out
  void* d_pow = nullptr;                              // device copy of the call's power table + its temperatures
  std::vector<double> pow_host;                       // what d_pow holds
  // resident rounds (mzx_actor_set_resident; mzx_resident.h): games, log and bookkeeping on the device
  mzx_actor_resident* resident = nullptr;
};

namespace mzx {

inline double actor_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline void actor_grow_ring(mzx_actor* a, int64_t need) {
  if (need <= a->cap) return;
  const int64_t limit = (int64_t)a->max_moves + 1;
  int64_t cap = std::max<int64_t>(std::max<int64_t>(2 * a->cap, need), std::min<int64_t>(limit, 32));
  cap = std::min<int64_t>(cap, std::max<int64_t>(limit, need));
  const int64_t B = a->B, A = a->A, E = a->E;
  std::vector<float> obs((size_t)(cap * B * E));
  std::vector<int32_t> tp((size_t)(cap * B)), vis((size_t)(cap * B * A));
  std::vector<int64_t> act((size_t)(cap * B));
  std::vector<double> rew((size_t)(cap * B)), val((size_t)(cap * B));
  std::vector<uint8_t> mask(a->game->always_all_legal ? 0 : (size_t)(cap * B * A));
  if (a->cap > 0) {
    int64_t lo = a->round;
    for (int64_t s = 0; s < B; ++s) lo = std::min(lo, a->start[s]);
    for (int64_t q = lo; q < a->round; ++q) {
      const int64_t o = q % a->cap, n = q % cap;
      memcpy(&obs[(size_t)(n * B * E)], &a->r_obs[(size_t)(o * B * E)], sizeof(float) * (size_t)(B * E));
      memcpy(&tp[(size_t)(n * B)], &a->r_tp[(size_t)(o * B)], sizeof(int32_t) * (size_t)B);
      memcpy(&vis[(size_t)(n * B * A)], &a->r_vis[(size_t)(o * B * A)], sizeof(int32_t) * (size_t)(B * A));
      memcpy(&act[(size_t)(n * B)], &a->r_act[(size_t)(o * B)], sizeof(int64_t) * (size_t)B);
      memcpy(&rew[(size_t)(n * B)], &a->r_rew[(size_t)(o * B)], sizeof(double) * (size_t)B);
      memcpy(&val[(size_t)(n * B)], &a->r_val[(size_t)(o * B)], sizeof(double) * (size_t)B);
      if (!mask.empty()) memcpy(&mask[(size_t)(n * B * A)], &a->r_mask[(size_t)(o * B * A)], (size_t)(B * A));
    }
  }
  a->r_obs.swap(obs); a->r_tp.swap(tp); a->r_vis.swap(vis); a->r_act.swap(act); a->r_rew.swap(rew); a->r_val.swap(val);
  a->r_mask.swap(mask);
  a->cap = cap;
}

// positions of the group's games as the next search reads them
inline void actor_refresh(mzx_actor* a) {
  mzx_game* g = a->game;
  rng_parallel(a->bank, a->B, a->move.num_threads, [=](int lo, int hi) {
    g->legal_actions(lo, hi, a->legal.data());
    g->to_play(lo, hi, a->to_play.data());
  });
}

// the temperature of every slot's next move (self_play.py:151-157)
inline void actor_move_temps(mzx_actor* a, int32_t temperature_threshold) {
  for (int k = 0; k < a->B; ++k) {
    const int64_t moves_before = a->round - a->start[k];
    a->move_temps[k] = (temperature_threshold && moves_before + 1 >= temperature_threshold) ? 0.0 : a->temps[k];
  }
}

typedef int (*actor_retry_fn)(void* ctx, int32_t group, int32_t count, const int32_t* games);

struct RoundsArgs {
  double* phase;               // [6] accumulators (mzx_rounds::phase_seconds)
  double temperature;
  int32_t temperature_threshold;
  const double* pow_table; int32_t table_stride; const double* table_temperatures; int32_t num_temperatures;
  actor_retry_fn retry; void* retry_ctx;
};

// The group's draws of search number `counter` (mzx_draws.h): its slots are the streams; the action choice reads the
// temperatures inside the input block and the call's power table on the device, its temperatures behind the rows
// (actor_upload_pow).  The legal rows, noise, tape and visit counts are the move's own (actor_queue_device_move).
inline void actor_draws(const mzx_actor* a, const RoundsArgs& args, uint64_t counter, mzx_draws* d, mzx_draws_select* sel) {
  *d = mzx_draws{};
  d->seed = a->draw_seed; d->counter = counter; d->first_stream = a->streams[0];
  d->num_games = a->B; d->action_space_size = a->A; d->tape_words = a->move.tape_words; d->dirichlet_alpha = a->move.dirichlet_alpha;
  *sel = mzx_draws_select{};
  sel->d_temperature = a->d_temperature; sel->d_action = a->d_action;
  if (args.num_temperatures > 0) {
    sel->d_pow_table = (const double*)a->d_pow;
    sel->d_table_temperatures = (const double*)a->d_pow + (size_t)args.num_temperatures * args.table_stride;
    sel->table_stride = args.table_stride; sel->num_temperatures = args.num_temperatures;
  }
}

// Draws into the move's noise and tape, the search, the action choice on its legal rows and visit counts (sel NULL: none):
// queued on `stream`, nothing uploaded, downloaded or waited for.
inline int actor_queue_device_move(mzx_search* s, const mzx_move* m, const mzx_draws* d, const mzx_draws_select* sel, void* d_arena,
                                   int64_t arena_bytes, void* stream) {
  const mzx_search_io& io = m->io;
  mzx_draws dd = *d;
  dd.d_legal_actions = io.d_legal_actions; dd.d_n = nullptr; dd.d_noise = (double*)io.d_noise; dd.d_tape = (uint32_t*)io.d_tape;
  dd.dirichlet_alpha = m->dirichlet_alpha;
  int rc = mzx_selfplay_draws(&dd, stream);
  if (rc == MZX_OK) rc = mzx_search_run(s, &io, d_arena, arena_bytes, stream);
  if (rc || !sel) return rc;
  mzx_draws_select ss = *sel;
  ss.d_legal_actions = io.d_legal_actions; ss.d_visit_counts = io.d_visit_counts;
  return mzx_selfplay_select_device(&dd, &ss, stream);
}

// the device-draws move of a group: temperatures into the input block, then upload, draws, search, action choice and
// download behind one call (mzx_selfplay_move_device); no host stream is touched
inline int actor_begin_device(mzx_actor* a, const RoundsArgs& args, void* stream) {
  actor_move_temps(a, args.temperature_threshold);
  memcpy(move_in_host(&a->move, a->d_temperature), a->move_temps.data(), sizeof(double) * (size_t)a->B);
  mzx_draws d; mzx_draws_select sel;
  actor_draws(a, args, a->draw_counter, &d, &sel);
  const int rc = mzx_selfplay_move_device(a->search, &a->move, &d, &sel, a->n_legal.data(), a->d_arena, a->arena_bytes, stream);
  if (rc == MZX_OK) ++a->draw_counter;
  return rc;
}

inline int actor_begin(mzx_actor* a, const RoundsArgs& args, void* stream, double* search_seconds, double* phase) {
  const double t0 = actor_now();
  mzx_move& m = a->move;
  m.streams = a->streams.data();
  m.legal_actions = a->legal.data();
  m.to_play = a->to_play.data();
  m.observation = a->cur_obs.data();
  m.observation_floats = a->E;
  m.flags = MZX_MOVE_NO_SYNC;
  int rc = a->device_draws ? actor_begin_device(a, args, stream)
                           : mzx_selfplay_search(a->search, a->bank, &m, a->n_legal.data(), a->d_arena, a->arena_bytes, stream);
  if (rc) return rc;
  rc = event_record(&a->event, (stream_t)stream);
  if (rc) { set_error("mzx_selfplay_rounds: event record failed: %s", runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  a->pending = true;
  const double dt = actor_now() - t0;
  *search_seconds += dt;
  phase[0] += dt;
  return MZX_OK;
}

// copies the games of slots idx (ascending) that ended with round r out of the ring
inline void actor_harvest(mzx_actor* a, const std::vector<int32_t>& idx, int64_t r, int64_t* sequence) {
  const int64_t B = a->B, A = a->A, E = a->E, cap = a->cap;
  mzx_actor::Batch b;
  int64_t rows = 0;
  for (int32_t s : idx) rows += r - a->start[s] + 1;
  const int64_t k = (int64_t)idx.size();
  b.slot.resize(k); b.n.resize(k); b.seq.resize(k);
  b.obs.resize((size_t)((rows + k) * E)); b.act.resize((size_t)(rows + k)); b.tp.resize((size_t)(rows + k));
  b.rew.resize((size_t)(rows + k)); b.vis.resize((size_t)(rows * A)); b.val.resize((size_t)rows);
  const bool masks = !a->r_mask.empty();
  bool any_illegal = false;
  if (masks) b.mask.resize((size_t)(rows * A));
  std::vector<int64_t> off1((size_t)k), off0((size_t)k);     // offsets of game j in the (n + 1)-long and n-long arrays
  int64_t o1 = 0, o0 = 0;
  for (int64_t j = 0; j < k; ++j) {
    const int32_t s = idx[j];
    const int64_t n = r - a->start[s] + 1;
    b.slot[j] = a->first_slot + s; b.n[j] = (int32_t)n; b.seq[j] = (*sequence)++;
    off1[j] = o1; off0[j] = o0;
    o1 += n + 1; o0 += n;
  }
  mzx_actor::Batch* bp = &b;
  std::vector<uint8_t> flag((size_t)k, 0);
  uint8_t* flagp = flag.data();
  const int64_t* p1 = off1.data();
  const int64_t* p0 = off0.data();
  const int32_t* idxp = idx.data();
  rng_parallel(a->bank, (int)k, a->move.num_threads, [=](int lo, int hi) {
    for (int j = lo; j < hi; ++j) {
      const int32_t s = idxp[j];
      const int64_t st = a->start[s], n = r - st + 1, q1 = p1[j], q0 = p0[j];
      bp->act[(size_t)q1] = 0; bp->rew[(size_t)q1] = 0.0;        // action_history / reward_history start with 0 (self_play.py:118-120)
      for (int64_t t = 0; t < n; ++t) {
        const int64_t c = (st + t) % cap;
        memcpy(&bp->obs[(size_t)((q1 + t) * E)], &a->r_obs[(size_t)((c * B + s) * E)], sizeof(float) * (size_t)E);
        bp->tp[(size_t)(q1 + t)] = a->r_tp[(size_t)(c * B + s)];
        bp->act[(size_t)(q1 + t + 1)] = a->r_act[(size_t)(c * B + s)];
        bp->rew[(size_t)(q1 + t + 1)] = a->r_rew[(size_t)(c * B + s)];
        memcpy(&bp->vis[(size_t)((q0 + t) * A)], &a->r_vis[(size_t)((c * B + s) * A)], sizeof(int32_t) * (size_t)A);
        bp->val[(size_t)(q0 + t)] = a->r_val[(size_t)(c * B + s)];
        if (masks) {
          const uint8_t* mk = &a->r_mask[(size_t)((c * B + s) * A)];
          memcpy(&bp->mask[(size_t)((q0 + t) * A)], mk, (size_t)A);
          for (int64_t x = 0; x < A; ++x) if (!mk[x]) flagp[j] = 1;
        }
      }
      // the position after the last move: its observation and side to move close the record (self_play.py:166-168)
      memcpy(&bp->obs[(size_t)((q1 + n) * E)], &a->next_obs[(size_t)(s * E)], sizeof(float) * (size_t)E);
      bp->tp[(size_t)(q1 + n)] = a->to_play[s];
    }
  });
  for (int64_t j = 0; j < k; ++j) any_illegal = any_illegal || flag[(size_t)j];
  if (masks && !any_illegal) { b.mask.clear(); b.mask.shrink_to_fit(); }
  std::lock_guard<std::mutex> lk(a->finished_lock);
  a->finished.push_back(std::move(b));
}

// the call's power table on the device (uploaded when it differs from what the actor holds; blocking, before any search)
inline int actor_upload_pow(mzx_actor* a, const RoundsArgs& args) {
  if (!a->device_draws || args.num_temperatures < 1) return MZX_OK;
  const size_t n = (size_t)args.num_temperatures * args.table_stride, total = n + (size_t)args.num_temperatures;
  std::vector<double> want(total);
  memcpy(want.data(), args.pow_table, sizeof(double) * n);
  memcpy(want.data() + n, args.table_temperatures, sizeof(double) * (size_t)args.num_temperatures);
  if (a->d_pow && want.size() == a->pow_host.size() && memcmp(want.data(), a->pow_host.data(), sizeof(double) * total) == 0) return MZX_OK;
  if (a->d_pow) { device_free(a->d_pow); a->d_pow = nullptr; a->pow_host.clear(); }
  if (device_alloc(&a->d_pow, sizeof(double) * total) != 0) { a->d_pow = nullptr; set_error("mzx_selfplay_rounds: power table allocation failed"); return MZX_ERR_RUNTIME; }
  if (copy_h2d_blocking(a->d_pow, want.data(), sizeof(double) * total) != 0) { set_error("mzx_selfplay_rounds: power table upload failed"); return MZX_ERR_RUNTIME; }
  a->pow_host.swap(want);
  return MZX_OK;
}

struct ActorRows {             // host rows [B] of a searched move: what an action re-drawn on the host reads and writes
  const int32_t* legal; const int32_t* visits; const double* temperature; int64_t* action;
};

// The tape repair of a searched move, `info` [B][4] being the host copy of what the search reported.  A tree that exhausted
// its tie-break tape is searched again on a longer one (rare: equal priors at every level): the retry callback owns that
// path (another staging geometry) and writes the results into the group's host output block.  Any flag left afterwards is
// an error.  On device draws the device chose the actions; the games searched again (`redo`) take theirs by the same
// function on the host, under the search's `counter`.
inline int actor_retry_flagged(const mzx_actor* a, int group, const RoundsArgs& args, const int32_t* info, uint64_t counter,
                               const ActorRows& rows, std::vector<int32_t>* redo) {
  const int B = a->B;
  for (int k = 0; k < B; ++k) if (info[4 * k + 1] & 1) redo->push_back(k);
  if (!redo->empty()) {
    if (!args.retry) { set_error("mzx_selfplay_rounds: a search exhausted its tie-break tape and no retry callback was given"); return MZX_ERR_RUNTIME; }
    const int rc = args.retry(args.retry_ctx, group, (int32_t)redo->size(), redo->data());
    if (rc) { set_error("mzx_selfplay_rounds: the tape-retry callback failed (%d)", rc); return MZX_ERR_RUNTIME; }
  }
  for (int k = 0; k < B; ++k)
    if (info[4 * k + 1] != 0) { set_error("search flagged tree %d (flags %d): node arena exhausted", k, info[4 * k + 1]); return MZX_ERR_RUNTIME; }
  if (!a->device_draws || redo->empty()) return MZX_OK;
  SelfplaySelectParams sp{};
  sp.seed = a->draw_seed; sp.counter = counter; sp.first_stream = a->streams[0];
  sp.legal = rows.legal; sp.visits = rows.visits; sp.temperature = rows.temperature; sp.pow_table = args.pow_table;
  sp.table_temperatures = args.table_temperatures; sp.action = rows.action; sp.B = B; sp.A = a->A;
  sp.table_stride = args.table_stride; sp.num_temperatures = args.num_temperatures;
  for (int32_t k : *redo) rows.action[k] = draw_select_action(sp, (size_t)k);
  return MZX_OK;
}

inline int actor_consume(mzx_actor* a, int group, const RoundsArgs& args, int64_t* sequence, int64_t* games_done,
                         double* search_seconds) {
  const double t0 = actor_now();
  if (!a->pending) { set_error("mzx_selfplay_rounds: no search in flight for group %d", group); return MZX_ERR_INVALID; }
  int rc = event_wait(a->event);
  if (rc) { set_error("mzx_selfplay_rounds: waiting for the search failed: %s", runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  a->pending = false;
  double t1 = actor_now();
  *search_seconds += t1 - t0;
  args.phase[1] += t1 - t0;
  const int B = a->B, A = a->A;
  const int64_t E = a->E;
  const mzx_move& m = a->move;
  const int32_t* info = move_out_host(&m, m.io.d_info);
  const int32_t* visits = move_out_host(&m, m.io.d_visit_counts);
  const double* root_value = move_out_host(&m, m.io.d_root_value);
  const bool dev = a->device_draws;
  actor_move_temps(a, args.temperature_threshold);
  if (dev) memcpy(a->actions.data(), move_out_host(&m, a->d_action), sizeof(int64_t) * (size_t)B);      // the device chose the actions
  std::vector<int32_t> redo;
  rc = actor_retry_flagged(a, group, args, info, a->draw_counter - 1, ActorRows{a->legal.data(), visits, a->move_temps.data(), a->actions.data()}, &redo);
  if (rc) return rc;
  if (!redo.empty()) { const double t2 = actor_now(); args.phase[4] += t2 - t1; t1 = t2; }
  const int64_t r = a->round;
  if (!dev) for (int k = 0; k < B; ++k) a->words[k] = info[4 * k + 2];      // (what the host streams consume; device draws consume nothing)
  if (A > 4096) { set_error("mzx_selfplay_rounds: more than 4096 actions"); return MZX_ERR_INVALID; }
  // (host draws: what select_range indexes; device draws: the same table rows and bounds the device's choice relied on)
  rc = select_check(a->legal.data(), a->n_legal.data(), visits, a->move_temps.data(), B, A, args.table_stride, args.table_temperatures,
                    args.num_temperatures);
  if (rc) return rc;
  int64_t lo_start = r;
  for (int k = 0; k < B; ++k) lo_start = std::min(lo_start, a->start[k]);
  actor_grow_ring(a, r - lo_start + 1);
  const int64_t c = r % a->cap;
  SelectArgs sa;
  sa.r = a->bank; sa.idx = a->streams.data(); sa.legal_all = a->legal.data(); sa.n_legal = a->n_legal.data(); sa.words = a->words.data();
  sa.visit_counts = visits; sa.temperature = a->move_temps.data(); sa.pow_table = args.pow_table; sa.table_stride = args.table_stride;
  sa.table_temperatures = args.table_temperatures; sa.num_temperatures = args.num_temperatures; sa.action = a->actions.data(); sa.A = A;
  mzx_game* g = a->game;
  const bool masks = !a->r_mask.empty();
  const int max_moves = a->max_moves;
  // ONE region per move and slot group: per game [lo, hi) the action draw (the stream consumes the search's tie words first),
  // the move's row of the log -- position searched (observation, side to move), action, search statistics, legal set --,
  // Game.step, the reward, and the next position (observation, side to move, legal actions) for the next search
  rng_parallel(a->bank, B, m.num_threads, [=](int lo, int hi) {
    if (!dev) select_range(sa, lo, hi);
    const size_t n = (size_t)(hi - lo);
    memcpy(&a->r_obs[(size_t)((c * B + lo) * E)], &a->cur_obs[(size_t)lo * E], sizeof(float) * n * (size_t)E);
    memcpy(&a->r_tp[(size_t)(c * B + lo)], &a->to_play[lo], sizeof(int32_t) * n);
    memcpy(&a->r_act[(size_t)(c * B + lo)], &a->actions[lo], sizeof(int64_t) * n);
    memcpy(&a->r_vis[(size_t)((c * B + lo) * A)], visits + (size_t)lo * A, sizeof(int32_t) * n * (size_t)A);
    memcpy(&a->r_val[(size_t)(c * B + lo)], root_value + lo, sizeof(double) * n);
    if (masks) {
      uint8_t* mk = &a->r_mask[(size_t)((c * B + lo) * A)];
      memset(mk, 0, n * (size_t)A);
      for (int k = lo; k < hi; ++k)
        for (int j = 0; j < a->n_legal[k]; ++j) mk[(size_t)(k - lo) * A + a->legal[(size_t)k * A + j]] = 1;
    }
    g->step(lo, hi, a->actions.data(), nullptr, a->reward.data(), a->done.data());
    memcpy(&a->r_rew[(size_t)(c * B + lo)], &a->reward[lo], sizeof(double) * n);
    g->observe(lo, hi, a->next_obs.data());
    g->to_play(lo, hi, a->to_play.data());
    g->legal_actions(lo, hi, a->legal.data());
    for (int k = lo; k < hi; ++k)
      if ((r - a->start[k]) + 2 > max_moves) a->done[k] = 1;        // len(action_history) <= max_moves, self_play.py:129
  });
  { const double t2 = actor_now(); args.phase[2] += t2 - t1; t1 = t2; }
  std::vector<int32_t> over;
  for (int k = 0; k < B; ++k)
    if (a->done[k]) over.push_back(k);
  if (!over.empty()) {
    actor_harvest(a, over, r, sequence);
    *games_done += (int64_t)over.size();
    g->reset(over.data(), (int32_t)over.size());          // the slots' next games begin (self_play.py:31-52)
    // first positions of the restarted slots, run by run of consecutive slots
    for (size_t q = 0; q < over.size();) {
      size_t e = q + 1;
      while (e < over.size() && over[e] == over[e - 1] + 1) ++e;
      const int lo = over[q], hi = over[e - 1] + 1;
      g->observe(lo, hi, a->next_obs.data());
      g->to_play(lo, hi, a->to_play.data());
      g->legal_actions(lo, hi, a->legal.data());
      q = e;
    }
    for (int32_t s : over) {
      a->start[s] = r + 1;
      a->temps[s] = args.temperature;
    }
  }
  a->cur_obs.swap(a->next_obs);
  args.phase[3] += actor_now() - t1;
  a->round = r + 1;
  return MZX_OK;
}

// The host loop of a rounds call: SelfPlay._rounds_batched, statement for statement.
inline int actor_rounds(mzx_actor* const* groups, int num_groups, const mzx_rounds* io, const RoundsArgs& args,
                        const std::vector<void*>& streams, int64_t* finished, int64_t* rounds, int64_t* searches, int64_t* sequence,
                        double* search_seconds) {
  int rc = MZX_OK;
  while (rc == MZX_OK && *finished < io->min_games && (io->max_rounds < 0 || *rounds < io->max_rounds)) {
    for (int k = 0; k < num_groups && rc == MZX_OK; ++k)
      if (!groups[k]->pending) rc = actor_begin(groups[k], args, streams[(size_t)k], search_seconds, args.phase);
    for (int k = 0; k < num_groups && rc == MZX_OK; ++k) {
      rc = actor_consume(groups[k], k, args, sequence, finished, search_seconds);
      if (rc) break;
      *searches += groups[k]->B;
      int64_t later = 0;
      for (int j = k + 1; j < num_groups; ++j) later += groups[j]->B;
      // certain to be consumed by this call: runs while the host plays the groups after it
      if (k + 1 < num_groups && *finished + later < io->min_games && (io->max_rounds < 0 || *rounds + 1 < io->max_rounds))
        rc = actor_begin(groups[k], args, streams[(size_t)k], search_seconds, args.phase);
    }
    ++*rounds;
  }
  return rc;
}

}  // namespace mzx
