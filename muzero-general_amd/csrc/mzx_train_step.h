// mzx_train_step.h -- what mzx_train_fc_step and mzx_train_resnet_step share (host only): the loss head's share of the
// scratch, the refusals both entries make before anything is launched, and the mzx_trainer_loss_io of a step.  The kernels
// and the rest of the plans are each trainer's own (mzx_train_fc.h, mzx_train_resnet.h).
#pragma once
#include <stddef.h>
#include <string.h>

#include <string>

#include "mzx_net.h"
#include "mzx_trainer.h"

namespace mzx {

// The front reads both io structs through mzx_train_fc_io: mzx_train_resnet_io is that struct with d_stats behind it.
#define MZX_TRAIN_IO_SAME(field) \
  static_assert(offsetof(mzx_train_fc_io, field) == offsetof(mzx_train_resnet_io, field), "mzx_train_*_io: " #field " moved")
MZX_TRAIN_IO_SAME(d_flat); MZX_TRAIN_IO_SAME(d_observation); MZX_TRAIN_IO_SAME(d_action); MZX_TRAIN_IO_SAME(d_target_value);
MZX_TRAIN_IO_SAME(d_target_reward); MZX_TRAIN_IO_SAME(d_target_policy); MZX_TRAIN_IO_SAME(d_gradient_scale);
MZX_TRAIN_IO_SAME(d_weight); MZX_TRAIN_IO_SAME(batch); MZX_TRAIN_IO_SAME(steps); MZX_TRAIN_IO_SAME(value_loss_weight);
MZX_TRAIN_IO_SAME(per_alpha); MZX_TRAIN_IO_SAME(d_grad_flat); MZX_TRAIN_IO_SAME(d_losses); MZX_TRAIN_IO_SAME(d_priorities);
MZX_TRAIN_IO_SAME(d_value_logits); MZX_TRAIN_IO_SAME(d_reward_logits); MZX_TRAIN_IO_SAME(d_policy_logits);
MZX_TRAIN_IO_SAME(d_scratch); MZX_TRAIN_IO_SAME(scratch_bytes);
#undef MZX_TRAIN_IO_SAME
static_assert(offsetof(mzx_train_resnet_io, d_stats) == sizeof(mzx_train_fc_io), "mzx_train_resnet_io: d_stats follows the common fields");

// The loss head's part of a step's plan: action count, support bins, and the scratch offsets (floats) of the loss rows, of
// d loss / d logit and of the logits the caller did not pass (-1: the caller's buffer).  FctPlan and RtnPlan begin with it.
struct TrainHeadPlan {
  int32_t A, F;
  int64_t off_loss, off_gv, off_gr, off_gp, off_vlog, off_rlog, off_plog;
};

// The first blocks of the scratch, for rows = B * steps; H.A and H.F are set.  take(floats) -> offset of the next block.
template <class Take>
inline void train_head_take(TrainHeadPlan& H, Take take, int64_t rows, bool own_vlog, bool own_rlog, bool own_plog) {
  H.off_loss = take(rows * (int64_t)(sizeof(TrainerLossRow) / 4));
  H.off_gv = take(rows * H.F); H.off_gr = take(rows * H.F); H.off_gp = take(rows * H.A);
  H.off_vlog = own_vlog ? take(rows * H.F) : -1;
  H.off_rlog = own_rlog ? take(rows * H.F) : -1;
  H.off_plog = own_plog ? take(rows * H.A) : -1;
}

// What `of` makes of the plan of a step that keeps all three logits in its scratch; 0 for a step the kernels do not run.
template <class Plan, class PlanFn, class Of>
inline int64_t train_full_plan(PlanFn plan, const mzx_net* net, int32_t batch, int32_t steps, Of of) {
  Plan P;
  return plan(net, batch, steps, true, true, true, P, nullptr) ? (int64_t)of(P) : 0;
}

// Every refusal of a step entry, in order, and its plan; nothing has been launched when this returns MZX_ERR_INVALID.
// need_stats: `io` is the prefix of a mzx_train_resnet_io, whose d_stats is required as well.
template <class Plan, class PlanFn>
inline int train_step_front(const char* who, const mzx_net* net, const mzx_train_fc_io* io, bool need_stats, PlanFn plan, Plan& P) {
  if (!net || !io) { set_error("%s: null argument", who); return MZX_ERR_INVALID; }
  if (io->batch < 1 || io->steps < 1) {
    set_error("%s: batch %d and steps %d must be positive", who, io->batch, io->steps);
    return MZX_ERR_INVALID;
  }
  if (!io->d_flat || !io->d_observation || !io->d_action || !io->d_target_value || !io->d_target_reward || !io->d_target_policy ||
      !io->d_gradient_scale || !io->d_grad_flat || !io->d_losses || !io->d_priorities || !io->d_scratch ||
      (need_stats && !reinterpret_cast<const mzx_train_resnet_io*>(io)->d_stats)) {
    set_error("%s: missing buffer", who);
    return MZX_ERR_INVALID;
  }
  std::string why;
  if (!plan(net, io->batch, io->steps, !io->d_value_logits, !io->d_reward_logits, !io->d_policy_logits, P, &why)) {
    set_error("%s: %s", who, why.c_str());
    return MZX_ERR_INVALID;
  }
  if (io->scratch_bytes < P.total_floats * 4 || ((uintptr_t)io->d_scratch % 16) != 0) {
    set_error("%s: scratch needs %lld bytes, 16-byte aligned", who,
              (long long)train_full_plan<Plan>(plan, net, io->batch, io->steps, [](const Plan& full) { return full.total_floats * 4; }));
    return MZX_ERR_INVALID;
  }
  // (the loss head's own argument checks, made here so that nothing is launched before a refusal)
  if (P.A < 1 || net->cfg.support_size < 0 || (int64_t)io->batch * io->steps >= ((int64_t)1 << 31)) {
    set_error("%s: shape out of range", who);
    return MZX_ERR_INVALID;
  }
  return MZX_OK;
}

// The loss head's call of a planned step, and where the step's logits go: the caller's buffer if given, else the scratch.
inline mzx_trainer_loss_io train_head_io(const mzx_train_fc_io* io, const TrainHeadPlan& H, float* scratch, int32_t support_size,
                                         float*& vlog, float*& rlog, float*& plog) {
  vlog = io->d_value_logits ? io->d_value_logits : scratch + H.off_vlog;
  rlog = io->d_reward_logits ? io->d_reward_logits : scratch + H.off_rlog;
  plog = io->d_policy_logits ? io->d_policy_logits : scratch + H.off_plog;
  mzx_trainer_loss_io lio;
  memset(&lio, 0, sizeof(lio));
  lio.d_value_logits = vlog; lio.d_reward_logits = rlog; lio.d_policy_logits = plog;
  lio.d_target_value = io->d_target_value; lio.d_target_reward = io->d_target_reward; lio.d_target_policy = io->d_target_policy;
  lio.d_gradient_scale = io->d_gradient_scale; lio.d_weight = io->d_weight;
  lio.batch = io->batch; lio.steps = io->steps; lio.support_size = support_size; lio.num_actions = H.A;
  lio.value_loss_weight = io->value_loss_weight; lio.per_alpha = io->per_alpha;
  lio.d_losses = io->d_losses; lio.d_priorities = io->d_priorities;
  lio.d_grad_value = scratch + H.off_gv; lio.d_grad_reward = scratch + H.off_gr; lio.d_grad_policy = scratch + H.off_gp;
  lio.d_scratch = scratch + H.off_loss; lio.scratch_bytes = mzx_trainer_loss_scratch_bytes(io->batch, io->steps);
  return lio;
}

}  // namespace mzx
