// mzx_selfplay.h -- the host side of ONE self-play move of a shard, shared by mzx_selfplay_search, mzx_selfplay_select and
// mzx_selfplay_move_device (mzx_lib.cpp) and by the round loops (mzx_actor.h, mzx_resident.h): addresses inside the two
// staged blocks of an mzx_move (Block), the staging of a move (move_check / move_stage / move_upload / move_finish), the
// argument checks of the device draws, and SelfPlay.select_action on the host streams (select_check / select_range).
// An entry keeps what is its own: host draws and the tape peek (mzx_selfplay_search), the move / draws agreement and the
// device sequence (mzx_selfplay_move_device; actor_queue_device_move, mzx_actor.h).
#pragma once
#include "mzx_draws.h"
#include "mzx_rng.h"
#include "mzx_search.h"

namespace mzx {

// a staged block: device address, host mirror (the same address on a build without a device), size
struct Block {
  const void* d; void* h; int64_t bytes;
  bool holds(const void* p, size_t n = 1) const {
    const ptrdiff_t off = (const char*)p - (const char*)d;
    return p && off >= 0 && off + (ptrdiff_t)n <= bytes;
  }
  // host address of the field whose device address is `p` (NULL when it lies outside the block)
  template <class T>
  T* host(const T* p) const { return holds(p) ? (T*)((char*)h + ((const char*)p - (const char*)d)) : nullptr; }
};
inline Block move_in(const mzx_move* m) { return {m->d_in, m->h_in, m->in_bytes}; }
inline Block move_out(const mzx_move* m) { return {m->d_out, m->h_out, m->out_bytes}; }
template <class T>
inline T* move_in_host(const mzx_move* m, const T* d) { return move_in(m).host(d); }
template <class T>
inline T* move_out_host(const mzx_move* m, const T* d) { return move_out(m).host(d); }

struct Carver {               // consecutive 16-byte aligned pieces of one allocation
  size_t at = 0;
  size_t take(size_t bytes) { const size_t o = at; at += (bytes + 15) & ~(size_t)15; return o; }
};

inline int rng_check(const mzx_rng* r, const int32_t* idx, int32_t count) {
  if (!r || (count > 0 && !idx) || count < 0) { set_error("rng: null / negative argument"); return MZX_ERR_INVALID; }
  const int32_t n = (int32_t)r->streams.size();
  for (int32_t k = 0; k < count; ++k)
    if (idx[k] < 0 || idx[k] >= n) { set_error("rng: stream index %d out of range (%d streams)", idx[k], n); return MZX_ERR_INVALID; }
  return MZX_OK;
}

inline int move_check(const mzx_rng* r, const mzx_move* m) {
  if (!m) { set_error("mzx_move: null"); return MZX_ERR_INVALID; }
  if (m->num_games < 1 || m->action_space_size < 1 || m->tape_words < 0) { set_error("mzx_move: sizes"); return MZX_ERR_INVALID; }
  if (!m->legal_actions) { set_error("mzx_move: legal_actions missing"); return MZX_ERR_INVALID; }
  return rng_check(r, m->streams, m->num_games);
}

// The staging of a move, for both entries (`who`): buffers present, io fields inside the staged input block -- with
// `host_draws` also the tape and, exactly with add_exploration_noise, the noise the host is about to write there --, the
// padded legal rows validated (n_legal filled), legal rows, to_play and observation copied into the block.
inline int move_stage(const mzx_move* m, int32_t* n_legal, const char* who, bool host_draws) {
  if (!n_legal || !m->legal_actions || !m->to_play || !m->h_in || !m->d_in || !m->h_out || !m->d_out || m->in_bytes < 1 ||
      m->out_bytes < 1) {
    set_error("%s: missing buffer", who);
    return MZX_ERR_INVALID;
  }
  const int B = m->num_games, A = m->action_space_size;
  const mzx_search_io& io = m->io;
  int32_t* h_legal = move_in_host(m, io.d_legal_actions);
  int32_t* h_to_play = move_in_host(m, io.d_to_play);
  float* h_obs = move_in_host(m, io.d_observation);
  if (!h_legal || !h_to_play || (m->observation && !h_obs) || (!m->observation && !io.d_observation) ||
      (host_draws && ((m->tape_words > 0 && !move_in_host(m, io.d_tape)) ||
                      (m->add_exploration_noise ? !move_in_host(m, io.d_noise) : io.d_noise != nullptr)))) {
    set_error("%s: io fields must lie inside the staged input block", who);
    return MZX_ERR_INVALID;
  }
  // self_play.py:296-301 on the padded lists
  for (int k = 0; k < B; ++k) {
    const int32_t* row = m->legal_actions + (size_t)k * A;
    int n = 0;
    while (n < A && row[n] >= 0) ++n;
    if (n == 0) { set_error("Legal actions should not be an empty array. Got [] (game %d).", k); return MZX_ERR_INVALID; }
    for (int j = 0; j < A; ++j)
      if (j < n ? row[j] >= A : row[j] >= 0) {
        set_error("Legal actions should be a subset of the action space (padded with -1 at the end); game %d.", k);
        return MZX_ERR_INVALID;
      }
    n_legal[k] = n;
  }
  memcpy(h_legal, m->legal_actions, sizeof(int32_t) * (size_t)B * A);
  memcpy(h_to_play, m->to_play, sizeof(int32_t) * (size_t)B);
  if (m->observation) memcpy(h_obs, m->observation, sizeof(float) * (size_t)B * m->observation_floats);
  return MZX_OK;
}

inline int move_upload(const mzx_move* m, void* stream) {
  if (m->h_in != m->d_in) MZX_TRY_LAUNCH(copy_h2d(m->d_in, m->h_in, (size_t)m->in_bytes, (stream_t)stream));
  return MZX_OK;
}

// the download of the output block and, without MZX_MOVE_NO_SYNC, the wait for it
inline int move_finish(const mzx_move* m, void* stream) {
  if (m->h_out != m->d_out) MZX_TRY_LAUNCH(copy_d2h(m->h_out, m->d_out, (size_t)m->out_bytes, (stream_t)stream));
  if (!(m->flags & MZX_MOVE_NO_SYNC)) MZX_TRY_LAUNCH(stream_sync((stream_t)stream));
  return MZX_OK;
}

// ---- device draws (mzx_draws.h): argument checks

inline int draws_check(const char* who, const mzx_draws* d) {
  if (!d) { set_error("%s: null mzx_draws", who); return MZX_ERR_INVALID; }
  if (d->num_games < 1 || d->action_space_size < 1) { set_error("%s: num_games and action_space_size must be positive", who); return MZX_ERR_INVALID; }
  if (d->action_space_size > DRAWS_MAX_ACTIONS) {
    set_error("%s: %d actions, the device draws take at most %d", who, d->action_space_size, DRAWS_MAX_ACTIONS);
    return MZX_ERR_INVALID;
  }
  return MZX_OK;
}

inline int draws_select_params(const char* who, const mzx_draws* d, const mzx_draws_select* sel, SelfplaySelectParams* p,
                               bool rows_of_move = false) {
  const int rc = draws_check(who, d);
  if (rc) return rc;
  if (!sel) { set_error("%s: null mzx_draws_select", who); return MZX_ERR_INVALID; }
  if ((!rows_of_move && (!sel->d_legal_actions || !sel->d_visit_counts)) || !sel->d_temperature || !sel->d_action) {
    set_error("%s: d_legal_actions, d_visit_counts, d_temperature and d_action are required", who);
    return MZX_ERR_INVALID;
  }
  if (sel->num_temperatures < 0 ||
      (sel->num_temperatures > 0 && (!sel->d_pow_table || !sel->d_table_temperatures || sel->table_stride < 1))) {
    set_error("%s: power table missing", who);
    return MZX_ERR_INVALID;
  }
  p->seed = d->seed; p->counter = d->counter; p->streams = d->d_streams; p->legal = sel->d_legal_actions;
  p->visits = sel->d_visit_counts; p->temperature = sel->d_temperature; p->pow_table = sel->d_pow_table;
  p->table_temperatures = sel->d_table_temperatures; p->uniforms = sel->d_uniforms; p->action = sel->d_action;
  p->first_stream = d->first_stream; p->B = d->num_games; p->A = d->action_space_size; p->table_stride = sel->table_stride;
  p->num_temperatures = sel->num_temperatures;
  return MZX_OK;
}

// ---- the action draw on the host streams

// SelfPlay.select_action (self_play.py:222-245) for the games [lo, hi) of a move: the streams first consume the tie-break
// words the search used (mzx_rng_advance), then every game's action is drawn.  Shared by mzx_selfplay_select and the round
// loop of mzx_actor.h (where it runs inside the per-move region together with the game step).
struct SelectArgs {
  mzx_rng* r; const int32_t* idx; const int32_t* legal_all; const int32_t* n_legal; const int32_t* words; const int32_t* visit_counts;
  const double* temperature; const double* pow_table; int32_t table_stride; const double* table_temperatures; int32_t num_temperatures;
  int64_t* action; int32_t A;
};

inline void select_range(const SelectArgs& s, int lo, int hi) {
  mzx_rng* r = s.r;
  const int32_t* idx = s.idx;
  const int A = s.A;
  double cdf[4096];
  for (int k = lo; k < hi; ++k) {
    rng_prefetch_next(r, idx, k, hi);
    Mt19937& g = r->streams[idx[k]];
    if (s.words) for (int32_t j = 0; j < s.words[k]; ++j) g.next32();        // what the search consumed (mzx_rng_advance)
    const int32_t* legal = s.legal_all + (size_t)k * A;
    const int32_t* vis = s.visit_counts + (size_t)k * A;
    const int n = s.n_legal[k];
    const double t = s.temperature[k];
    int pos = 0;
    if (t == 0.0) {                            // actions[numpy.argmax(visit_counts)]: the first maximum
      int32_t best = vis[legal[0]];
      for (int j = 1; j < n; ++j) if (vis[legal[j]] > best) { best = vis[legal[j]]; pos = j; }
    } else if (t == MZX_INF) {                 // numpy.random.choice(actions)
      pos = (int)g.bounded((uint32_t)n);
    } else {                                   // numpy.random.choice(actions, p=dist / sum(dist)): mzx_rng_choice_weighted
      int row = 0;
      for (int q = 0; q < s.num_temperatures; ++q) if (s.table_temperatures[q] == t) row = q;
      const double* tab = s.pow_table + (size_t)row * s.table_stride;
      double total = 0.0;
      for (int j = 0; j < n; ++j) total = total + tab[vis[legal[j]]];
      double acc = 0.0;
      for (int j = 0; j < n; ++j) { acc = acc + tab[vis[legal[j]]] / total; cdf[j] = acc; }
      const double last = cdf[n - 1];
      const double u = g.next_double();
      for (int j = 0; j < n; ++j) pos += (cdf[j] / last <= u) ? 1 : 0;
    }
    s.action[k] = legal[pos < n ? pos : n - 1];
  }
}

// the argument checks of mzx_selfplay_select (temperatures have a power table row, visit counts lie inside it)
inline int select_check(const int32_t* legal_all, const int32_t* n_legal, const int32_t* visit_counts, const double* temperature,
                        int B, int A, int32_t table_stride, const double* table_temperatures, int32_t num_temperatures) {
  for (int k = 0; k < B; ++k) {
    if (n_legal[k] < 1 || n_legal[k] > A) { set_error("n_legal[%d] = %d out of range", k, n_legal[k]); return MZX_ERR_INVALID; }
    const double t = temperature[k];
    if (t == 0.0 || t == MZX_INF) continue;
    int row = -1;
    for (int q = 0; q < num_temperatures; ++q) if (table_temperatures[q] == t) row = q;
    if (row < 0) { set_error("mzx_selfplay_select: no power table for temperature %g", t); return MZX_ERR_INVALID; }
    const int32_t* legal = legal_all + (size_t)k * A;
    const int32_t* vis = visit_counts + (size_t)k * A;
    for (int j = 0; j < n_legal[k]; ++j)
      if (vis[legal[j]] < 0 || vis[legal[j]] >= table_stride) { set_error("visit count %d outside the power table", vis[legal[j]]); return MZX_ERR_INVALID; }
  }
  return MZX_OK;
}

}  // namespace mzx
