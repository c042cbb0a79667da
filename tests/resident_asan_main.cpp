// resident_asan_main.cpp -- a stand-alone program (its own main) that plays RESIDENT rounds on the serial build of the
// library with the address and undefined-behaviour sanitizers watching: the harvest, offset, log-wrap and gather
// indexing of csrc/mzx_resident.h is where an out-of-range index would become a GPU fault, so it is walked on the CPU
// first.  Built and run by tests/test_resident_rounds_asan.py:
//     g++ -fsanitize=address,undefined -DMZX_HOSTCHECK -x c++ tests/resident_asan_main.cpp
// Two shards, two slot groups each, chunk = 3 (calls straddle chunk ends, the log ring wraps many times):
//   synthetic (2, 1, 3), 3 actions, 2 players, 12 games, max_moves 5 on a fully connected network: rounds 7 + 6;
//   tic-tac-toe, 5 games on a small residual network: rounds 13 + 14 + 13.
// Weights are filled deterministically.  The tape-retry path stays out (its callback lives in Python): the tape is long
// enough that no search of these shards exhausts it, and a halt without a callback would fail the run.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

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
  }
}

// plays the calls, takes the finished games of every call, returns how many games finished
int64_t play(Shard& sh, int sims, const std::vector<int>& calls, int A, int64_t E, int64_t* rounds_out) {
  std::vector<double> table((size_t)sims + 2), temps(1, 1.0);
  for (size_t c = 0; c < table.size(); ++c) table[c] = (double)c;       // visit_count ** (1 / 1.0)
  mzx_actor* handles[2] = {sh.groups[0].actor, sh.groups[1].actor};
  int64_t sequence = 0, games = 0, rounds = 0;
  for (int max_rounds : calls) {
    mzx_rounds io{};
    io.temperature = 1.0; io.temperature_threshold = 4; io.table_stride = sims + 2; io.pow_table = table.data();
    io.table_temperatures = temps.data(); io.num_temperatures = 1; io.min_games = (int64_t)1 << 60; io.max_rounds = max_rounds;
    io.sequence = sequence;
    CHECK(mzx_selfplay_rounds(handles, 2, &io, nullptr));
    if (io.rounds != max_rounds) { fprintf(stderr, "played %lld rounds of %d\n", (long long)io.rounds, max_rounds); exit(1); }
    sequence = io.sequence; rounds += io.rounds;
    for (mzx_actor* a : handles) {
      int64_t counts[3];
      CHECK(mzx_actor_finished(a, sequence, counts));
      const size_t G = (size_t)counts[0], rows = (size_t)counts[1];
      if (G == 0) continue;
      std::vector<int32_t> slot(G), length(G), vis(rows * (size_t)A);
      std::vector<int64_t> seq(G), act(rows + G), tp(rows + G);
      std::vector<float> obs((rows + G) * (size_t)E);
      std::vector<double> rew(rows + G), val(rows);
      std::vector<uint8_t> mask(rows * (size_t)A);
      int32_t illegal = 0;
      CHECK(mzx_actor_take(a, sequence, slot.data(), length.data(), seq.data(), obs.data(), act.data(), rew.data(), tp.data(), vis.data(),
                           val.data(), mask.data(), &illegal));
      size_t total = 0;
      for (size_t j = 0; j < G; ++j) {
        if (length[j] < 1 || seq[j] < 0 || seq[j] >= sequence) { fprintf(stderr, "game %zu: length %d sequence %lld\n", j, length[j], (long long)seq[j]); exit(1); }
        total += (size_t)length[j];
      }
      if (total != rows) { fprintf(stderr, "lengths sum to %zu, %zu rows\n", total, rows); exit(1); }
      games += (int64_t)G;
    }
  }
  for (mzx_actor* a : handles) {
    int64_t st[8];
    CHECK(mzx_actor_resident_stats(a, st));
    if (st[0] != rounds || st[2] != 0) { fprintf(stderr, "committed %lld of %lld rounds, %lld repairs\n", (long long)st[0], (long long)rounds, (long long)st[2]); exit(1); }
  }
  *rounds_out = rounds;
  return games;
}

void close_shard(Shard& sh) {
  for (Group& G : sh.groups) { mzx_actor_destroy(G.actor); mzx_search_destroy(G.search); mzx_game_destroy(G.game); }
  mzx_rng_destroy(sh.bank);
  mzx_net_destroy(sh.net);
}

}  // namespace

int main() {
  int64_t rounds = 0;
  {
    mzx_net_config nc{};
    nc.network = 0; nc.observation_shape[0] = 2; nc.observation_shape[1] = 1; nc.observation_shape[2] = 3;
    nc.action_space_size = 3; nc.support_size = 10; nc.encoding_size = 8;
    nc.n_fc_dynamics_layers = 1; nc.fc_dynamics_layers[0] = 16; nc.n_fc_reward_layers = 1; nc.fc_reward_layers[0] = 16;
    nc.n_fc_value_layers = 1; nc.fc_value_layers[0] = 16; nc.n_fc_policy_layers = 1; nc.fc_policy_layers[0] = 16;
    Shard sh;
    make_shard(sh, nc, "synthetic", 12, 2, 7, 5, 64);
    const int64_t games = play(sh, 7, {7, 6}, 3, 6, &rounds);
    printf("synthetic: %lld rounds, %lld games\n", (long long)rounds, (long long)games);
    if (games != 24) { fprintf(stderr, "expected 24 games of 5 moves\n"); return 1; }
    close_shard(sh);
  }
  {
    mzx_net_config nc{};
    nc.network = 1; nc.observation_shape[0] = 3; nc.observation_shape[1] = 3; nc.observation_shape[2] = 3;
    nc.action_space_size = 9; nc.support_size = 10; nc.encoding_size = 32; nc.blocks = 1; nc.channels = 8;
    nc.reduced_channels_reward = 4; nc.reduced_channels_value = 4; nc.reduced_channels_policy = 4;
    nc.n_resnet_fc_reward_layers = 1; nc.resnet_fc_reward_layers[0] = 8; nc.n_resnet_fc_value_layers = 1; nc.resnet_fc_value_layers[0] = 8;
    nc.n_resnet_fc_policy_layers = 1; nc.resnet_fc_policy_layers[0] = 8;
    Shard sh;
    make_shard(sh, nc, "tictactoe", 5, 2, 8, 9, 64);
    const int64_t games = play(sh, 8, {13, 14, 13}, 9, 27, &rounds);
    printf("tictactoe: %lld rounds, %lld games\n", (long long)rounds, (long long)games);
    if (games < 20) { fprintf(stderr, "expected at least 20 games in 40 rounds of 5 slots\n"); return 1; }
    close_shard(sh);
  }
  printf("ok\n");
  return 0;
}
