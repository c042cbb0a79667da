// mzx_train_chain.h -- what mzx_train_chain (include/mzx.h) adds to the entries it queues: the carve of its one workspace
// and the small kernel between mzx_replay_batch and the training step.  The chain itself (mzx_lib.cpp) calls the entries
// a caller would call, step after step on one stream: mzx_replay_sample, mzx_replay_batch, ChainPrepOp,
// mzx_train_fc_step / mzx_train_resnet_step, the optimizer launch (mzx_optim.h), mzx_train_resnet_commit_stats,
// mzx_replay_update_priorities; behind the last step mzx_net_set_weights.  Every step reuses the same blocks: the stream
// orders them.
#pragma once
#include "mzx_launch.h"
#include "mzx_net.h"

namespace mzx {

// The conversions mzx.replay.trainer_tensors and mzx.trainer._train_gradients make with torch between a gathered batch and
// a step: value / reward / policy f64 -> f32, gradient scale i64 -> f32 (all round-to-nearest-even), action i64 -> i32.
struct ChainPrepOp {
  const double* value; const double* reward; const double* policy;
  const int64_t* scale; const int64_t* action;
  float* value_out; float* reward_out; float* policy_out; float* scale_out;
  int32_t* action_out;
  int64_t rows;      // batch x (unroll steps + 1)
  int32_t A;
  MZX_HD size_t size() const { return (size_t)(rows * (A + 4)); }
  MZX_HD void operator()(size_t i) const {
    int64_t k = (int64_t)i;
    if (k < rows * A) { policy_out[k] = (float)policy[k]; return; }
    k -= rows * A;
    if (k < rows) { value_out[k] = (float)value[k]; return; }
    k -= rows;
    if (k < rows) { reward_out[k] = (float)reward[k]; return; }
    k -= rows;
    if (k < rows) { scale_out[k] = (float)scale[k]; return; }
    k -= rows;
    action_out[k] = (int32_t)action[k];
  }
};

// Byte offsets of the blocks of the workspace, each 256-byte aligned.
struct ChainPlan {
  int64_t base, game_id, len, pos, tape, weight, obs, value64, reward64, policy64, action64, scale64;
  int64_t value, reward, policy, scale, action, priorities, stats, scratch, step_scratch_bytes, total_bytes;
};

// rows = batch x steps; step_scratch_bytes / stat_floats: the training step's own (0 stat floats for a fully connected network)
inline ChainPlan chain_plan(const mzx_net* net, int32_t batch, int32_t steps, int64_t step_scratch_bytes, int64_t stat_floats) {
  ChainPlan P;
  int64_t at = 0;
  auto take = [&](int64_t bytes) { const int64_t off = at; at += (bytes + 255) / 256 * 256; return off; };
  const int64_t B = batch, rows = B * steps, A = net->cfg.action_space_size;
  P.base = take(B * 8); P.game_id = take(B * 8); P.len = take(B * 4); P.pos = take(B * 4); P.tape = take(rows * 4);
  P.weight = take(B * 4);
  P.obs = take(B * net->input_size * 4);
  P.value64 = take(rows * 8); P.reward64 = take(rows * 8); P.policy64 = take(rows * A * 8);
  P.action64 = take(rows * 8); P.scale64 = take(rows * 8);
  P.value = take(rows * 4); P.reward = take(rows * 4); P.policy = take(rows * A * 4); P.scale = take(rows * 4);
  P.action = take(rows * 4);
  P.priorities = take(rows * 4);
  P.stats = take(stat_floats * 4);
  P.scratch = take(step_scratch_bytes);
  P.step_scratch_bytes = step_scratch_bytes;
  P.total_bytes = at;
  return P;
}

}  // namespace mzx
