// handoff_asan_main.cpp -- a stand-alone program (its own main) that walks the PIECE LIFETIME of the device hand-off
// (mzx_actor_set_device_handoff, csrc/mzx_resident.h) on the serial build of the library with the address and
// undefined-behaviour sanitizers watching: recycling, release, harvest into released buffers, destroy with pieces
// outstanding -- where a host bug would become a GPU fault.  Built and run by tests/test_device_handoff_asan.py:
//     g++ -fsanitize=address,undefined -DMZX_HOSTCHECK -x c++ tests/handoff_asan_main.cpp
// A tic-tac-toe shard of 5 games in two hand-off groups, chunk = 3, plays 10 calls over many chunk ends.  Every call's
// pieces are taken and ingested into a small replay pool by mzx_replay_ingest reading the piece's own arrays and columns
// (the pool is a ring of a few hundred rows: games overwrite older ones), one game per piece is exported again
// (mzx_replay_export) and compared with a download of the piece (mzx_actor_download_device), the pieces are released and
// the next call harvests into their buffers.  The last call's pieces stay outstanding -- some taken and never released,
// some never taken -- and the actors are destroyed with them.  The shard set-up is that of tests/resident_asan_main.cpp.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../muzero-general_amd/csrc/mzx_lib.cpp"

#define CHECK(expr)                                                                              \
  do {                                                                                           \
    const int rc_ = (expr);                                                                      \
    if (rc_ != 0) { fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #expr, rc_, mzx_last_error()); exit(1); } \
  } while (0)

namespace {

struct Unit {                 // uniform numbers in [0, 1), the same on every run
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

struct Group {
  std::vector<char> h_in, d_in, h_out, d_out, arena;
  std::vector<double> noise;
  std::vector<uint32_t> tape;
  std::vector<int32_t> streams;
  mzx_game* game = nullptr;
  mzx_search* search = nullptr;
  mzx_actor* actor = nullptr;
};

struct Shard {
  mzx_net* net = nullptr;
  std::vector<float> flat, derived;
  std::vector<double> pbc, sq;
  mzx_rng* bank = nullptr;
  std::vector<Group> groups;
};

void make_shard(Shard& sh, const mzx_net_config& nc, const char* kind, int B, int players, int sims, int max_moves, int tape_words) {
  CHECK(mzx_net_create(&nc, &sh.net));
  const int64_t n = mzx_net_num_params(sh.net);
  sh.flat.resize((size_t)n);
  Unit u{12345};
  for (int32_t t = 0; t < mzx_net_num_tensors(sh.net); ++t) {
    char name[256];
    int64_t off = 0, numel = 0;
    int32_t dims[4];
    CHECK(mzx_net_tensor_info(sh.net, t, name, sizeof(name), &off, &numel, dims));
    const bool variance = strstr(name, "running_var") != nullptr;
    for (int64_t i = 0; i < numel; ++i) sh.flat[(size_t)(off + i)] = variance ? (float)(0.5 + u.next()) : (float)(0.6 * (u.next() - 0.5));
  }
  sh.derived.resize((size_t)mzx_net_derived_floats(sh.net) + 1);
  CHECK(mzx_net_set_weights(sh.net, sh.flat.data(), n, sh.derived.data(), mzx_net_derived_floats(sh.net), nullptr));
  for (int k = 0; k <= sims; ++k) { sh.pbc.push_back(log((k + 19652.0 + 1) / 19652.0) + 1.25); sh.sq.push_back(sqrt((double)k)); }
  CHECK(mzx_rng_create(B, &sh.bank));
  std::vector<uint32_t> seeds((size_t)B);
  for (int k = 0; k < B; ++k) seeds[(size_t)k] = 100u + (uint32_t)k;
  CHECK(mzx_rng_seed(sh.bank, 0, B, seeds.data()));
  const int A = nc.action_space_size;
  const int64_t E = (int64_t)nc.observation_shape[0] * nc.observation_shape[1] * nc.observation_shape[2];
  sh.groups.resize(2);
  const int edges[3] = {0, (B + 1) / 2, B};
  for (int g = 0; g < 2; ++g) {
    Group& G = sh.groups[(size_t)g];
    const int first = edges[g], nb = edges[g + 1] - edges[g];
    CHECK(mzx_game_create(kind, nb, seeds.data() + first, nc.observation_shape, A, players, &G.game));
    mzx_search_config sc{};
    sc.num_trees = nb; sc.num_simulations = sims; sc.action_space_size = A; sc.num_players = players; sc.support_size = nc.support_size;
    sc.tape_words = tape_words; sc.discount = 0.997; sc.root_exploration_fraction = 0.25;
    sc.h_pb_c_table = sh.pbc.data(); sc.h_sqrt_table = sh.sq.data();
    CHECK(mzx_search_create(&sc, sh.net, &G.search));
    G.arena.resize((size_t)mzx_search_arena_bytes(G.search));
    // the staged blocks: [temperature f64 | obs f32 | legal i32 | to_play i32] and [root f64 | predicted f64 | action i64 | visits i32 | info i32]
    const size_t in_bytes = 8 * (size_t)nb + 4 * (size_t)(nb * E) + 4 * (size_t)(nb * A) + 4 * (size_t)nb;
    const size_t out_bytes = 24 * (size_t)nb + 4 * (size_t)(nb * A) + 16 * (size_t)nb;
    G.h_in.assign(in_bytes, 0); G.d_in.assign(in_bytes, 0); G.h_out.assign(out_bytes, 0); G.d_out.assign(out_bytes, 0);
    G.noise.assign((size_t)(nb * A), 0.0); G.tape.assign((size_t)(nb * tape_words), 0u);
    for (int k = 0; k < nb; ++k) G.streams.push_back(first + k);
    mzx_actor_config ac{};
    ac.game = G.game; ac.search = G.search; ac.bank = sh.bank; ac.streams = G.streams.data(); ac.first_slot = first;
    ac.max_moves = max_moves; ac.temperature = 1.0; ac.d_arena = G.arena.data(); ac.arena_bytes = (int64_t)G.arena.size();
    mzx_move& m = ac.move;
    m.num_games = nb; m.action_space_size = A; m.tape_words = tape_words; m.num_threads = 1; m.dirichlet_alpha = 0.25;
    m.add_exploration_noise = 1;
    m.h_in = G.h_in.data(); m.d_in = G.d_in.data(); m.in_bytes = (int64_t)in_bytes;
    m.h_out = G.h_out.data(); m.d_out = G.d_out.data(); m.out_bytes = (int64_t)out_bytes;
    char* din = G.d_in.data();
    char* dout = G.d_out.data();
    double* d_temperature = (double*)din;
    m.io.d_observation = (const float*)(din + 8 * (size_t)nb);
    m.io.d_legal_actions = (const int32_t*)(din + 8 * (size_t)nb + 4 * (size_t)(nb * E));
    m.io.d_to_play = (const int32_t*)(din + 8 * (size_t)nb + 4 * (size_t)(nb * E) + 4 * (size_t)(nb * A));
    m.io.d_noise = G.noise.data(); m.io.d_tape = G.tape.data();
    m.io.d_root_value = (double*)dout; m.io.d_root_predicted_value = (double*)(dout + 8 * (size_t)nb);
    int64_t* d_action = (int64_t*)(dout + 16 * (size_t)nb);
    m.io.d_visit_counts = (int32_t*)(dout + 24 * (size_t)nb);
    m.io.d_info = (int32_t*)(dout + 24 * (size_t)nb + 4 * (size_t)(nb * A));
    CHECK(mzx_actor_create(&ac, &G.actor));
    CHECK(mzx_actor_set_device_draws(G.actor, 0x1234567ull, 0, d_temperature, d_action));
    CHECK(mzx_actor_set_resident(G.actor, 3, (int64_t)1 << 30));
    CHECK(mzx_actor_set_device_handoff(G.actor, 1));
  }
}


struct Pool {                 // a small replay pool with a sampler, rows allocated round-robin from a ring
  int64_t rows; int A, F, slots;
  std::vector<float> frames, priorities, slot_priority;
  std::vector<int32_t> actions, to_play, owner, slot_len;
  std::vector<double> rewards, root_values, child_visits, values, slot_sum, tile_prefix, raw, discount_pow;
  std::vector<int64_t> slot_game, slot_base;
  std::vector<uint32_t> mask;
  mzx_replay_pool pool{};
  mzx_replay_sampler sampler{};
  int64_t head = 0, next_id = 0;
  Pool(int64_t rows_, int A_, int C, int H, int W, int slots_) : rows(rows_), A(A_), F(C * H * W), slots(slots_) {
    frames.assign((size_t)(rows * F), 0.f); priorities.assign((size_t)rows, 0.f); slot_priority.assign((size_t)slots, 0.f);
    actions.assign((size_t)rows, 0); to_play.assign((size_t)rows, 0); owner.assign((size_t)rows, -1); slot_len.assign((size_t)slots, 0);
    rewards.assign((size_t)rows, 0.0); root_values.assign((size_t)rows, 0.0); child_visits.assign((size_t)(rows * A), 0.0);
    values.assign((size_t)rows, 0.0); slot_sum.assign((size_t)slots, 0.0); tile_prefix.assign(2 * (size_t)((slots + 255) / 256), 0.0);
    raw.assign(1, 0.0); slot_game.assign((size_t)slots, -1); slot_base.assign((size_t)slots, 0);
    mask.assign((size_t)(rows * ((A + 31) / 32)), 0u);
    for (int i = 0; i <= 4; ++i) discount_pow.push_back(pow(0.997, i));
    pool.d_frames = frames.data(); pool.d_actions = actions.data(); pool.d_rewards = rewards.data(); pool.d_to_play = to_play.data();
    pool.d_root_values = root_values.data(); pool.d_child_visits = child_visits.data(); pool.d_values = values.data();
    pool.rows = rows; pool.channels = C; pool.height = H; pool.width = W; pool.action_space_size = A;
    sampler.d_priorities = priorities.data(); sampler.d_owner = owner.data(); sampler.d_slot_game = slot_game.data();
    sampler.d_slot_base = slot_base.data(); sampler.d_slot_len = slot_len.data(); sampler.d_slot_priority = slot_priority.data();
    sampler.d_slot_sum = slot_sum.data(); sampler.rows = rows; sampler.slots = slots; sampler.d_tile_prefix = tile_prefix.data();
    sampler.d_raw = raw.data(); sampler.raw_capacity = 1;
  }
  int64_t place(int32_t T) {                        // T + 1 contiguous rows, wrapping to row 0
    if (head + T + 1 > rows) head = 0;
    const int64_t base = head;
    head += T + 1;
    return base;
  }
};

int64_t pieces_taken = 0;

int fail(const char* what) { fprintf(stderr, "%s: %s\n", what, mzx_last_error()); exit(1); }

// takes the pieces of one group numbered below `before`; ingest + export + download + release unless `keep`
int64_t hand_over(mzx_actor* a, int64_t before, Pool& P, int A, int64_t E, bool keep, std::vector<int64_t>* kept_tokens) {
  int64_t counts[2], got[2];
  CHECK(mzx_actor_finished_device(a, before, counts));
  const size_t NP = (size_t)counts[0], G = (size_t)counts[1];
  if (NP == 0) return 0;
  std::vector<int64_t> info(NP * MZX_PIECE_INFO_WORDS), seq(G);
  std::vector<int32_t> slot(G), length(G);
  CHECK(mzx_actor_take_device(a, before, (int32_t)NP, (int64_t)G, info.data(), slot.data(), length.data(), seq.data(), got));
  if (got[0] != counts[0] || got[1] != counts[1]) fail("take_device handed out other counts than finished_device");
  // a second take finds nothing, the host-path entries refuse a hand-off group
  CHECK(mzx_actor_finished_device(a, before, counts));
  if (counts[0] != 0) fail("pieces left behind a take");
  int64_t three[3];
  if (mzx_actor_finished(a, before, three) != MZX_ERR_INVALID) fail("mzx_actor_finished accepted a hand-off group");
  size_t g0 = 0;
  pieces_taken += (int64_t)NP;
  for (size_t p = 0; p < NP; ++p) {
    const int64_t* row = info.data() + p * MZX_PIECE_INFO_WORDS;
    const int64_t token = row[0];
    const size_t k = (size_t)row[1], rows0 = (size_t)row[2], rows1 = rows0 + k;
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) {
      if (length[g0 + j] < 1 || seq[g0 + j] < 0 || seq[g0 + j] >= before) fail("a game's length or sequence");
      total += (size_t)length[g0 + j];
    }
    if (total != rows0) fail("lengths do not sum to the piece's rows");
    if (keep) { kept_tokens->push_back(token); g0 += k; continue; }
    // the piece on the host, for the comparison below
    std::vector<float> obs(rows1 * (size_t)E);
    std::vector<int64_t> act(rows1), tp(rows1);
    std::vector<double> rew(rows1), val(rows0);
    std::vector<int32_t> vis(rows0 * (size_t)A);
    std::vector<uint8_t> mask(rows0 * (size_t)A);
    CHECK(mzx_actor_download_device(a, token, obs.data(), act.data(), rew.data(), tp.data(), vis.data(), val.data(),
                                    row[3] ? mask.data() : nullptr, nullptr));
    // one ingest whose columns and staged arrays point into the piece; the last game of every piece is passed over
    std::vector<int64_t> base(k), ids(k);
    for (size_t j = 0; j < k; ++j) { base[j] = j + 1 == k && k > 1 ? -1 : P.place(length[g0 + j]); ids[j] = P.next_id++; }
    mzx_replay_ingest_io io{};
    io.d_len = (const int32_t*)row[4]; io.d_src1 = (const int64_t*)row[5]; io.d_src0 = (const int64_t*)row[6];
    io.d_base = base.data(); io.d_game_id = ids.data();
    io.d_observations = (const float*)row[7]; io.d_actions = (const int64_t*)row[8]; io.d_rewards = (const double*)row[9];
    io.d_to_play = (const int64_t*)row[10]; io.d_visits = (const int32_t*)row[11]; io.d_root_values = (const double*)row[12];
    io.d_legal_mask = (const uint8_t*)row[13]; io.d_discount_pow = P.discount_pow.data(); io.per_alpha = 0.5;
    io.total_rows = (int64_t)rows1; io.num_games = (int32_t)k; io.td_steps = 4; io.per = 1; io.action_space_size = A;
    io.channels = P.pool.channels; io.height = P.pool.height; io.width = P.pool.width;
    CHECK(mzx_replay_ingest(&P.pool, &P.sampler, P.mask.data(), P.rows, &io, nullptr));
    // the first game of the piece read back from the pool: what the piece held
    const int32_t T = length[g0];
    std::vector<float> x_obs((size_t)(T + 1) * (size_t)E);
    std::vector<int64_t> x_act((size_t)T + 1), x_tp((size_t)T + 1);
    std::vector<double> x_rew((size_t)T + 1), x_cv((size_t)T * (size_t)A), x_val((size_t)T);
    std::vector<uint8_t> x_mask((size_t)T * (size_t)A);
    std::vector<float> x_pri((size_t)T);
    const int64_t zero = 0;
    mzx_replay_export_io xo{};
    xo.d_base = base.data(); xo.d_len = &length[g0]; xo.d_dst1 = &zero; xo.d_dst0 = &zero;
    xo.d_observations = x_obs.data(); xo.d_actions = x_act.data(); xo.d_rewards = x_rew.data(); xo.d_to_play = x_tp.data();
    xo.d_child_visits = x_cv.data(); xo.d_root_values = x_val.data(); xo.d_legal_mask = x_mask.data(); xo.d_priorities = x_pri.data();
    xo.total_rows = T + 1; xo.num_games = 1;
    CHECK(mzx_replay_export(&P.pool, &P.sampler, P.mask.data(), P.rows, &xo, nullptr));
    if (memcmp(x_obs.data(), obs.data(), sizeof(float) * x_obs.size()) != 0 || memcmp(x_act.data(), act.data(), 8 * x_act.size()) != 0 ||
        memcmp(x_rew.data(), rew.data(), 8 * x_rew.size()) != 0 || memcmp(x_tp.data(), tp.data(), 8 * x_tp.size()) != 0)
      fail("the exported game differs from the piece");
    for (size_t t = 0; t < (size_t)T; ++t) {
      int64_t sum = 0;
      for (int x = 0; x < A; ++x) sum += vis[t * (size_t)A + x];
      for (int x = 0; x < A; ++x) {
        const bool ok = !row[3] || mask[t * (size_t)A + x];
        const double want = sum > 0 && ok ? (double)vis[t * (size_t)A + x] / (double)sum : 0.0;
        if (x_cv[t * (size_t)A + x] != want || (row[3] && x_mask[t * (size_t)A + x] != mask[t * (size_t)A + x])) fail("child visits / mask of the exported game");
      }
      if (x_val[t] != (sum > 0 ? val[t] : 0.0)) fail("root value of the exported game");
    }
    CHECK(mzx_actor_release_device(a, token, nullptr));
    if (mzx_actor_release_device(a, token, nullptr) != MZX_ERR_INVALID) fail("a released token was accepted again");
    if (mzx_actor_download_device(a, token, obs.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != MZX_ERR_INVALID)
      fail("a released piece was downloaded");
    g0 += k;
  }
  return (int64_t)G;
}

}  // namespace

int main() {
  mzx_net_config nc{};
  nc.network = 1; nc.observation_shape[0] = 3; nc.observation_shape[1] = 3; nc.observation_shape[2] = 3;
  nc.action_space_size = 9; nc.support_size = 10; nc.encoding_size = 32; nc.blocks = 1; nc.channels = 8;
  nc.reduced_channels_reward = 4; nc.reduced_channels_value = 4; nc.reduced_channels_policy = 4;
  nc.n_resnet_fc_reward_layers = 1; nc.resnet_fc_reward_layers[0] = 8; nc.n_resnet_fc_value_layers = 1; nc.resnet_fc_value_layers[0] = 8;
  nc.n_resnet_fc_policy_layers = 1; nc.resnet_fc_policy_layers[0] = 8;
  const int sims = 8, A = 9;
  const int64_t E = 27;
  Shard sh;
  make_shard(sh, nc, "tictactoe", 5, 2, sims, 9, 64);
  Pool P(300, A, 3, 3, 3, 64);
  std::vector<double> table((size_t)sims + 2), temps(1, 1.0);
  for (size_t c = 0; c < table.size(); ++c) table[c] = (double)c;
  mzx_actor* handles[2] = {sh.groups[0].actor, sh.groups[1].actor};
  const int calls[10] = {7, 4, 9, 13, 1, 2, 14, 5, 8, 11};
  int64_t sequence = 0, games = 0, most = 0;
  std::vector<int64_t> kept;
  for (int c = 0; c < 10; ++c) {
    mzx_rounds io{};
    io.temperature = 1.0; io.temperature_threshold = 4; io.table_stride = sims + 2; io.pow_table = table.data();
    io.table_temperatures = temps.data(); io.num_temperatures = 1; io.min_games = (int64_t)1 << 60; io.max_rounds = calls[c];
    io.sequence = sequence;
    CHECK(mzx_selfplay_rounds(handles, 2, &io, nullptr));
    sequence = io.sequence;
    const bool last = c == 9;
    // the last call: group 0's pieces are taken and kept, group 1's are never taken
    for (int k = 0; k < 2; ++k)
      if (!last || k == 0) games += hand_over(handles[k], sequence, P, A, E, last, &kept);
    int64_t st[8], total = 0;
    for (mzx_actor* a : handles) { CHECK(mzx_actor_resident_stats(a, st)); total += st[7]; }
    // recycling: a call of at most 14 rounds is at most five chunks, so a group has at most five pieces out at once; the
    // buffers (128 KiB each at these sizes) are reused call after call instead of one being allocated per piece
    most = total > most ? total : most;
    if (total > 2 * 5 * ((int64_t)2 << 16)) { fprintf(stderr, "call %d: %lld bytes in pieces\n", c, (long long)total); return 1; }
  }
  if (pieces_taken * ((int64_t)2 << 16) <= 2 * most) { fprintf(stderr, "%lld pieces in %lld bytes: nothing was recycled\n", (long long)pieces_taken, (long long)most); return 1; }
  if (games < 20 || kept.empty()) { fprintf(stderr, "%lld games, %zu kept pieces\n", (long long)games, kept.size()); return 1; }
  int64_t left[2];
  CHECK(mzx_actor_finished_device(handles[1], -1, left));
  if (left[0] < 1) { fprintf(stderr, "group 1 has no piece queued at the end\n"); return 1; }
  if (mzx_actor_set_device_handoff(handles[1], 0) != MZX_ERR_INVALID) fail("the hand-off was switched off with pieces pending");
  printf("%lld games handed over, %zu pieces taken and kept, %lld queued at the destroy\n", (long long)games, kept.size(), (long long)left[0]);
  for (Group& G : sh.groups) { mzx_actor_destroy(G.actor); mzx_search_destroy(G.search); mzx_game_destroy(G.game); }
  mzx_rng_destroy(sh.bank);
  mzx_net_destroy(sh.net);
  printf("ok\n");
  return 0;
}
