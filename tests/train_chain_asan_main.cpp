// train_chain_asan_main.cpp -- a stand-alone program (its own main) that runs mzx_train_chain (csrc/mzx_train_chain.h) on the
// serial build of the library with the address and undefined-behaviour sanitizers watching: the chain carves ONE workspace
// into the blocks of the sampler, the gather, the conversions, the training step and the statistics, and every buffer
// here is a heap block of exactly the size the header asks for, so a block that is carved short or a launch that runs past
// its block is an error report, not a GPU fault later.  Built and run by tests/test_train_chain_asan.py:
//     g++ -fsanitize=address,undefined -DMZX_HOSTCHECK -x c++ tests/train_chain_asan_main.cpp
// A fully connected and a residual network, batch 5, three unroll steps, a pool of three games of 2, 6 and 4 positions
// (windows overlap and run past game ends), three chained steps each with and without PER, Adam and SGD with momentum.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../muzero-general_amd/csrc/mzx_lib.cpp"

#define CHECK(expr)                                                                              \
  do {                                                                                           \
    const int rc_ = (expr);                                                                      \
    if (rc_ != 0) { fprintf(stderr, "%s:%d: %s -> %d: %s\n", __FILE__, __LINE__, #expr, rc_, mzx_last_error()); exit(1); } \
  } while (0)
#define REQUIRE(cond)                                                                            \
  do {                                                                                           \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); exit(1); } \
  } while (0)

namespace {

struct Unit {                 // uniform numbers in [0, 1), the same on every run
  uint64_t s;
  double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
};

void run(const mzx_net_config& nc, int kind, bool per) {
  const int B = 5, U = 3, steps = U + 1, n_chain = 3, slots = 4;
  const int lengths[3] = {2, 6, 4};
  Unit u{777};
  mzx_net* net = nullptr;
  CHECK(mzx_net_create(&nc, &net));
  const int64_t n = mzx_net_num_params(net);
  std::vector<float> flat((size_t)n), grad((size_t)n, 0.f), m((size_t)n, 0.f), v((size_t)n, 0.f);
  std::vector<int64_t> spans;
  for (int32_t t = 0; t < mzx_net_num_tensors(net); ++t) {
    char name[256];
    int64_t off = 0, numel = 0;
    int32_t dims[4];
    CHECK(mzx_net_tensor_info(net, t, name, sizeof(name), &off, &numel, dims));
    const bool variance = strstr(name, "running_var") != nullptr, statistic = variance || strstr(name, "running_mean") != nullptr;
    for (int64_t i = 0; i < numel; ++i) flat[(size_t)(off + i)] = variance ? (float)(0.5 + u.next()) : (float)(0.6 * (u.next() - 0.5));
    if (!statistic) { spans.push_back(off); spans.push_back(numel); }
  }
  const int32_t num_spans = (int32_t)(spans.size() / 2);
  const int64_t num_chunks = mzx_optim_chunks(spans.data(), num_spans, n, nullptr, 0);
  REQUIRE(num_chunks > 0);
  std::vector<int64_t> chunks((size_t)(2 * num_chunks));
  REQUIRE(mzx_optim_chunks(spans.data(), num_spans, n, chunks.data(), num_chunks) == num_chunks);
  std::vector<float> derived((size_t)mzx_net_derived_floats(net));
  CHECK(mzx_net_set_weights(net, flat.data(), n, derived.data(), (int64_t)derived.size(), nullptr));

  // the pool: game g at rows base .. base + T, the sampler's table and priorities
  const int C = nc.observation_shape[0], H = nc.observation_shape[1], W = nc.observation_shape[2], A = nc.action_space_size;
  const int k = nc.stacked_observations;
  int64_t rows = 0;
  for (int T : lengths) rows += T + 1;
  std::vector<float> frames((size_t)(rows * C * H * W)), priorities((size_t)rows, 0.f), slot_priority(slots, 0.f);
  std::vector<int32_t> actions((size_t)rows), to_play((size_t)rows, 0), owner((size_t)rows, -1), slot_len(slots, 0), slot_list(slots);
  std::vector<double> rewards((size_t)rows), root_values((size_t)rows), values((size_t)rows), visits((size_t)(rows * A)), slot_sum(slots, 0.0);
  std::vector<int64_t> slot_game(slots, -1), slot_base(slots, 0);
  for (float& x : frames) x = (float)(u.next() - 0.5);
  for (int64_t r = 0; r < rows; ++r) {
    actions[(size_t)r] = (int32_t)(u.next() * A) % A;
    rewards[(size_t)r] = u.next() - 0.5; root_values[(size_t)r] = u.next() - 0.5; values[(size_t)r] = 2 * (u.next() - 0.5);
    for (int a = 0; a < A; ++a) visits[(size_t)(r * A + a)] = 1.0 / A;
  }
  int64_t base = 0, total_samples = 0;
  for (int g = 0; g < 3; ++g) {
    slot_game[(size_t)g] = g; slot_base[(size_t)g] = base; slot_len[(size_t)g] = lengths[g];
    for (int i = 0; i < lengths[g]; ++i) priorities[(size_t)(base + i)] = per ? (float)(0.1 + u.next()) : 0.f;
    base += lengths[g] + 1;
    total_samples += lengths[g];
  }
  for (int s = 0; s < slots; ++s) slot_list[(size_t)s] = s;
  mzx_replay_pool pool{};
  pool.d_frames = frames.data(); pool.d_actions = actions.data(); pool.d_rewards = rewards.data(); pool.d_to_play = to_play.data();
  pool.d_root_values = root_values.data(); pool.d_child_visits = visits.data(); pool.d_values = values.data();
  pool.rows = rows; pool.channels = C; pool.height = H; pool.width = W; pool.action_space_size = A;
  std::vector<double> tile_prefix((size_t)(2 * ((slots + 255) / 256))), raw((size_t)B);
  mzx_replay_sampler sampler{};
  sampler.d_priorities = priorities.data(); sampler.d_owner = owner.data(); sampler.d_slot_game = slot_game.data();
  sampler.d_slot_base = slot_base.data(); sampler.d_slot_len = slot_len.data(); sampler.d_slot_priority = slot_priority.data();
  sampler.d_slot_sum = slot_sum.data(); sampler.rows = rows; sampler.slots = slots;
  sampler.d_tile_prefix = tile_prefix.data(); sampler.d_raw = raw.data(); sampler.raw_capacity = B;
  CHECK(mzx_replay_sampler_refresh(&sampler, slot_list.data(), slots, nullptr));

  REQUIRE(mzx_train_chain_supported(net, B, steps) == 1);
  const int64_t bytes = mzx_train_chain_scratch_bytes(net, B, steps);
  REQUIRE(bytes > 0);
  // exactly `bytes` (a multiple of 256) on a 256-byte boundary: one byte further is a report
  REQUIRE(bytes % 256 == 0);
  char* workspace = (char*)aligned_alloc(256, (size_t)bytes);
  REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0);

  std::vector<float> losses((size_t)(4 * n_chain), -7.f);
  std::vector<double> lr(n_chain), ss(n_chain), bc(n_chain);
  for (int i = 0; i < n_chain; ++i) {
    lr[(size_t)i] = 0.02 * pow(0.8, (2 + i) / 3.0);
    ss[(size_t)i] = lr[(size_t)i] / (1 - pow(0.9, 1 + i));
    bc[(size_t)i] = sqrt(1 - pow(0.999, 1 + i));
  }
  mzx_train_chain_io io{};
  io.pool = &pool; io.sampler = &sampler; io.seed = 7; io.first_call = 8; io.total_samples = total_samples;
  io.per = per ? 1 : 0; io.num_unroll_steps = U; io.stacked_observations = k; io.num_actions = A;
  io.batch = B; io.num_steps = n_chain; io.value_loss_weight = 0.25; io.per_alpha = 0.5;
  io.d_flat = flat.data(); io.d_grad_flat = grad.data();
  io.optim.kind = kind; io.optim.first_step = 1; io.optim.t = 1;
  io.optim.d_param = flat.data(); io.optim.d_grad = grad.data(); io.optim.d_state1 = m.data(); io.optim.d_state2 = v.data();
  io.optim.n = n; io.optim.h_spans = spans.data(); io.optim.num_spans = num_spans; io.optim.d_chunks = chunks.data();
  io.optim.num_chunks = (int32_t)num_chunks;
  io.optim.weight_decay = 1e-4; io.optim.momentum = 0.9; io.optim.one_minus_beta1 = 1 - 0.9; io.optim.beta2 = 0.999;
  io.optim.one_minus_beta2 = 1 - 0.999; io.optim.eps = 1e-8;
  io.h_lr = lr.data(); io.h_step_size = ss.data(); io.h_bias_correction2_sqrt = bc.data();
  io.d_losses = losses.data(); io.d_derived = derived.data(); io.derived_floats = (int64_t)derived.size();
  io.d_workspace = workspace; io.workspace_bytes = bytes;
  const std::vector<float> before = flat;
  CHECK(mzx_train_chain(net, &io, nullptr));
  for (float x : losses) REQUIRE(isfinite(x) && x != -7.f);
  bool moved = false;
  for (size_t i = 0; i < flat.size(); ++i) { REQUIRE(isfinite(flat[i])); moved = moved || flat[i] != before[i]; }
  REQUIRE(moved);
  for (int32_t o : owner) REQUIRE(o == -1);
  // the refusals queue nothing: a workspace one byte short, a misaligned one
  mzx_train_chain_io bad = io;
  bad.workspace_bytes = bytes - 1;
  REQUIRE(mzx_train_chain(net, &bad, nullptr) == MZX_ERR_INVALID);
  bad = io;
  bad.d_workspace = workspace + 16;
  REQUIRE(mzx_train_chain(net, &bad, nullptr) == MZX_ERR_INVALID);
  bad = io;
  bad.optim.t = 0;
  REQUIRE(mzx_train_chain(net, &bad, nullptr) == MZX_ERR_INVALID);
  free(workspace);
  mzx_net_destroy(net);
}

}  // namespace

int main() {
  mzx_net_config fc{};
  fc.network = 0; fc.observation_shape[0] = 1; fc.observation_shape[1] = 2; fc.observation_shape[2] = 3; fc.stacked_observations = 2;
  fc.action_space_size = 3; fc.support_size = 4; fc.encoding_size = 6;
  fc.n_fc_dynamics_layers = 1; fc.fc_dynamics_layers[0] = 7; fc.n_fc_reward_layers = 1; fc.fc_reward_layers[0] = 5;
  fc.n_fc_value_layers = 1; fc.fc_value_layers[0] = 5; fc.n_fc_policy_layers = 1; fc.fc_policy_layers[0] = 5;
  mzx_net_config res{};
  res.network = 1; res.observation_shape[0] = 3; res.observation_shape[1] = 3; res.observation_shape[2] = 3;
  res.action_space_size = 9; res.support_size = 2; res.encoding_size = 8; res.blocks = 1; res.channels = 5;
  res.reduced_channels_reward = 2; res.reduced_channels_value = 2; res.reduced_channels_policy = 2;
  res.n_resnet_fc_reward_layers = 1; res.resnet_fc_reward_layers[0] = 4; res.n_resnet_fc_value_layers = 1; res.resnet_fc_value_layers[0] = 4;
  res.n_resnet_fc_policy_layers = 1; res.resnet_fc_policy_layers[0] = 4;
  for (const mzx_net_config* nc : {&fc, &res})
    for (int per = 0; per < 2; ++per) {
      run(*nc, MZX_OPTIM_ADAM, per != 0);
      run(*nc, MZX_OPTIM_SGD, per != 0);
    }
  printf("ok\n");
  return 0;
}
