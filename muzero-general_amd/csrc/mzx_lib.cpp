// mzx_lib.cpp -- the C ABI (include/mzx.h).  Compiled as HIP for gfx950 into
// libmzx.so (product) and, with -DMZX_HOSTCHECK, as plain C++ into the test-only
// libmzx_hostcheck.so.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <string>

#include "mzx_actor.h"
#include "mzx_draws.h"
#include "mzx_games_device.h"
#include "mzx_obs.h"
#include "mzx_optim.h"
#include "mzx_replay.h"
#include "mzx_resident.h"
#include "mzx_rng.h"
#include "mzx_search.h"
#include "mzx_selfplay.h"
#include "mzx_trainer.h"
#include "mzx_train_fc.h"
#include "mzx_train_resnet.h"
#include "mzx_train_chain.h"
#include "mzx_train_step.h"
#include "mzx_tree_carry.h"
#ifndef MZX_HOSTCHECK
#include "mzx_fused_fc.h"
#include "mzx_fused_fc2.h"
#include "mzx_resnet_search.h"
#include "mzx_row_search.h"
// rt_search_kernel and its planner: part of THIS translation unit (round 6).  As a unit of its own it instantiated every
// header-defined kernel a second time (648 kernels in both code objects: the library was 9.3 MB, half of it duplicates).
#include "mzx_tower_search.inc"
#endif

namespace mzx {

static thread_local std::string g_error;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_error = buf;
}

}  // namespace mzx

using namespace mzx;

extern "C" {

int mzx_abi_version(void) { return MZX_ABI_VERSION; }

const char* mzx_last_error(void) { return g_error.c_str(); }

int mzx_is_device_build(void) {
#ifdef MZX_HOSTCHECK
  return 0;
#else
  return 1;
#endif
}

// ---------------------------------------------------------------- network

int mzx_net_create(const mzx_net_config* cfg, mzx_net** out) {
  if (!cfg || !out) { set_error("mzx_net_create: null argument"); return MZX_ERR_INVALID; }
  const int32_t counts[] = {cfg->n_fc_representation_layers, cfg->n_fc_dynamics_layers, cfg->n_fc_reward_layers,
                            cfg->n_fc_value_layers, cfg->n_fc_policy_layers, cfg->n_resnet_fc_reward_layers,
                            cfg->n_resnet_fc_value_layers, cfg->n_resnet_fc_policy_layers};
  for (int32_t n : counts)
    if (n < 0 || n > MZX_MAX_LAYERS) { set_error("more than %d hidden layers in an MLP", MZX_MAX_LAYERS); return MZX_ERR_INVALID; }
  mzx_net* net = new (std::nothrow) mzx_net();
  if (!net) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  net->cfg = *cfg;
  NetBuilder b(net);
  if (!b.build()) { delete net; return MZX_ERR_INVALID; }
  rz_plan(net);
  rb_plan(net);
  *out = net;
  return MZX_OK;
}

void mzx_net_destroy(mzx_net* net) { delete net; }

int32_t mzx_net_num_tensors(const mzx_net* net) { return net ? (int32_t)net->tensors.size() : 0; }
int64_t mzx_net_num_params(const mzx_net* net) { return net ? net->num_params : 0; }
int64_t mzx_net_hidden_size(const mzx_net* net) { return net ? net->hidden_size : 0; }
int64_t mzx_net_input_size(const mzx_net* net) { return net ? net->input_size : 0; }
static int64_t derived_total(const mzx_net* net) {
  int64_t n = net->rz.ok ? net->rz.derived_floats : net->derived_floats;
  if (net->rb.ok && net->rb.derived_floats > n) n = net->rb.derived_floats;
  return n > 0 ? n : 1;
}
int64_t mzx_net_derived_floats(const mzx_net* net) { return net ? derived_total(net) : 0; }
int64_t mzx_net_workspace_floats(const mzx_net* net, int32_t max_batch) {
  if (!net || max_batch < 1) return 0;
  return net_ws_per_sample(net) * (int64_t)max_batch;
}

int mzx_net_tensor_info(const mzx_net* net, int32_t i, char* name, int32_t name_cap, int64_t* offset,
                        int64_t* numel, int32_t dims[4]) {
  if (!net || i < 0 || i >= (int32_t)net->tensors.size()) { set_error("tensor index out of range"); return MZX_ERR_INVALID; }
  const TensorInfo& t = net->tensors[i];
  if (name && name_cap > 0) { strncpy(name, t.name.c_str(), name_cap - 1); name[name_cap - 1] = 0; }
  if (offset) *offset = t.offset;
  if (numel) *numel = t.numel;
  if (dims) for (int k = 0; k < 4; ++k) dims[k] = t.dims[k];
  return MZX_OK;
}

int mzx_net_set_weights(mzx_net* net, const float* d_flat, int64_t n_floats, float* d_derived,
                        int64_t derived_floats, void* stream) {
  if (!net || !d_flat || !d_derived) { set_error("mzx_net_set_weights: null argument"); return MZX_ERR_INVALID; }
  if (n_floats != net->num_params) {
    set_error("flat weight buffer has %lld floats, network expects %lld", (long long)n_floats, (long long)net->num_params);
    return MZX_ERR_INVALID;
  }
  if (derived_floats < derived_total(net)) { set_error("derived buffer too small"); return MZX_ERR_WORKSPACE; }
  net->d_flat = d_flat;
  net->d_derived = d_derived;
  for (const BnRef& r : net->bns) {
    BnFoldOp op;
    op.weight = d_flat + r.weight; op.bias = d_flat + r.bias; op.mean = d_flat + r.mean; op.var = d_flat + r.var;
    op.alpha = d_derived + r.alpha; op.beta = d_derived + r.beta; op.channels = r.channels;
    MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  }
  if (net->rz.ok) {  // MFMA-fragment-ordered weights + program tables of the fused residual engine
    for (const RzPack& p : net->rz.packs) {
      RzPackOp op;
      op.W = d_flat + p.src; op.out = d_derived + p.dst;
      op.taps = p.taps; op.cin = p.cin; op.cin_total = p.cin_total; op.cchunks = p.cchunks; op.cout = p.cout;
      op.nchunks = p.nchunks; op.wchunks = p.wchunks; op.ntiles = p.ntiles;
      MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
    }
    for (const RzAsum& q : net->rz.asums) {
      RzAsumOp op;
      op.W = d_flat + q.src; op.out = d_derived + q.dst; op.cout = q.cout; op.cin_total = q.cin_total; op.H = q.H; op.Wd = q.W;
      MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
    }
    for (const RzCopy& c : net->rz.copies) {
      RzCopyOp op;
      op.src = (c.from_derived ? (const float*)d_derived : d_flat) + c.src; op.dst = d_derived + c.dst; op.n = c.n; op.npad = c.npad;
      MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
    }
    for (const RzProgram* R : {&net->rz.initial, &net->rz.recurrent})
      if (R->ok) {
        MZX_TRY_LAUNCH(copy_h2d(d_derived + R->small_base, R->ops, sizeof(RzOp) * R->n_ops, (stream_t)stream));
        MZX_TRY_LAUNCH(copy_h2d(d_derived + R->small_base + R->aoff_base, R->aoff.data(), sizeof(int32_t) * R->aoff.size(),
                                (stream_t)stream));
      }
  }
#ifndef MZX_HOSTCHECK
  if (net->rb.ok) {  // streamed MFMA engine: fragment-ordered weights, action tap sums
    const int rc = rb_refresh_derived(net, d_flat, d_derived, (stream_t)stream);
    if (rc) return rc;
  }
#endif
  return MZX_OK;
}

int mzx_net_fused_supported(const mzx_net* net) {
  if (!net || !net->rz.ok) return 0;
  return (net->rz.initial.ok ? 1 : 0) | (net->rz.recurrent.ok ? 2 : 0);
}

int mzx_net_streamed_supported(const mzx_net* net) {
  if (!net || !net->rb.ok) return 0;
  const bool fi = net->rz.ok && net->rz.initial.ok, fr = net->rz.ok && net->rz.recurrent.ok;
  return ((net->rb.initial.ok && !fi) ? 1 : 0) | ((net->rb.recurrent.ok && !fr) ? 2 : 0);
}

int mzx_net_streamed_plan(const mzx_net* net, int32_t recurrent, int32_t op, int32_t out[24]) {
  if (!net || !out) { set_error("null argument"); return MZX_ERR_INVALID; }
  const RbProgram& R = recurrent ? net->rb.recurrent : net->rb.initial;
  if (!net->rb.ok || !R.ok || op < 0 || op >= (int32_t)R.ops.size()) { set_error("no streamed plan for this operator"); return MZX_ERR_INVALID; }
  const RbOp& o = R.ops[op];
  const int32_t v[24] = {o.kind, o.in_layout, o.out_layout, o.res_layout, o.taps, o.stride, o.cin, o.cout, o.hin, o.win,
                         o.hout, o.wout, o.T, o.th, o.tw, o.tiles_x, o.tiles_y, o.PH, o.PW, o.cpg, o.phases, o.rows,
                         o.mtiles, o.lds_bytes};
  for (int k = 0; k < 24; ++k) out[k] = v[k];
  return MZX_OK;
}

int mzx_net_streamed_shape(const mzx_net* net, int32_t recurrent, int32_t op, int32_t batch, int32_t out[16]) {
  if (!net || !out || batch < 1) { set_error("null argument / batch < 1"); return MZX_ERR_INVALID; }
  const RbProgram& R = recurrent ? net->rb.recurrent : net->rb.initial;
  if (!net->rb.ok || !R.ok || op < 0 || op >= (int32_t)R.ops.size() || R.ops[op].kind != RB_GEMM) {
    set_error("operator %d has no streamed GEMM plan", op);
    return MZX_ERR_INVALID;
  }
  const RbShape sh = rb_choose_shape(R.ops[op], batch);
  const int32_t v[16] = {sh.T, sh.rows, sh.mtiles, sh.lds, sh.ntiles_wg, sh.nsplit, sh.NT, sh.WN, sh.WM, sh.MT, sh.groups,
                         sh.cpg, sh.phases, sh.Cs, R.ops[op].ntiles, R.ops[op].cchunks};
  for (int k = 0; k < 16; ++k) out[k] = v[k];
  return MZX_OK;
}

int mzx_net_streamed_tower(const mzx_net* net, int32_t recurrent, int32_t index, int32_t batch, int32_t out[16]) {
  if (!net || !out || batch < 1) { set_error("null argument / batch < 1"); return MZX_ERR_INVALID; }
  const RbProgram& R = recurrent ? net->rb.recurrent : net->rb.initial;
  if (!net->rb.ok || !R.ok || net->rb_no_towers || index < 0 || index >= (int32_t)R.towers.size()) {
    set_error("no tower %d", index);
    return MZX_ERR_INVALID;
  }
  const RbTower& tw = R.towers[index];
  const RbTowerShape sh = rb_tower_shape(tw, batch);
  // (groups = 0: at this batch the tower's layers launch one by one, rb_tower_use)
  const int32_t v[16] = {tw.first, tw.count, tw.C, tw.H, tw.W, sh.T, sh.MT, sh.NT, sh.WM, sh.WN, sh.lds,
                         rb_tower_use(tw, batch) ? sh.groups : 0, tune(TUNE_RB_TAIL) == 0 ? 0 : tw.n_tail, 0, 0, 0};
  for (int k = 0; k < 16; ++k) out[k] = v[k];
  return MZX_OK;
}

int mzx_net_streamed_heads(const mzx_net* net, int32_t recurrent, int32_t batch, int32_t out[16]) {
  if (!net || !out || batch < 1) { set_error("null argument / batch < 1"); return MZX_ERR_INVALID; }
  for (int k = 0; k < 16; ++k) out[k] = 0;
  const RbProgram& R = recurrent ? net->rb.recurrent : net->rb.initial;
  if (!net->rb.ok || !R.ok) return MZX_OK;
  const int mode = rb_heads_mode();
  if (net->rb_no_towers || tune(TUNE_RB_TAIL) == 0 || mode != 2) return MZX_OK;
  // out: [0] Linear operators that leave the layer-by-layer path, [1] chains, [2 .. 13] the operators, [14] their levels
  // inside their chains (2 bits each), [15] the mode (rb_heads_mode)
  int n = 0;
  for (int q = 0; q < R.heads.n_chains; ++q) {
    const RbHeadChain& hc = R.heads.chain[q];
    const int t = R.ops[hc.conv_op].tower_of_tail;
    if (t < 0 || !rb_tower_use(R.towers[t], batch)) continue;
    ++out[1];
    for (int l = 0; l < hc.count && n < 12; ++l) { out[14] |= l << (2 * n); out[2 + n++] = hc.first + l; }
  }
  out[0] = n;
  out[15] = n ? mode : 0;
  return MZX_OK;
}

int mzx_net_streamed_split(const mzx_net* net, int32_t batch, int32_t out[2]) {
  if (!net || !out || batch < 1) { set_error("null argument / batch < 1"); return MZX_ERR_INVALID; }
  const int first = rb_split_first(net, batch, tune(TUNE_ROW_SPLIT_MIN));
  out[0] = first > 0 ? first : batch;
  out[1] = first > 0 ? batch - first : 0;
  return MZX_OK;
}

int64_t mzx_net_operator_out_floats(const mzx_net* net, int32_t recurrent, int32_t op) {
  if (!net) return 0;
  const std::vector<OpDesc>& prog = recurrent ? net->prog_recurrent : net->prog_initial;
  if (op < 0 || op >= (int32_t)prog.size()) return 0;
  const OpDesc& d = prog[op];
  switch (d.kind) {      // (the sizes run_network_prefix copies out)
    case OP_LINEAR: return d.out_features;
    case OP_CONV3: case OP_POOL: case OP_CONVK: case OP_MAXPOOL: case OP_ADAPTIVE_POOL: return (int64_t)d.cout * d.hout * d.wout;
    case OP_CONV1: return (int64_t)d.cout * d.hin;
    default: return (int64_t)d.groups_per_sample * d.len;
  }
}

int mzx_net_set_mode(mzx_net* net, int32_t mode) {
  if (!net) { set_error("null network handle"); return MZX_ERR_INVALID; }
  if (mode < 0 || mode > 5) { set_error("network mode is 0 (one kernel per operator), 1 (fused engine, streamed engine for what it cannot hold), 2 (fused, 4-wave workgroups), 3 (streamed engine for everything), 4 (as 3, layer by layer: no tower launches) or 5 (as 1, the streamed engine layer by layer)"); return MZX_ERR_INVALID; }
  if ((mode == 3 || mode == 4) && !net->rb.ok) { set_error("the streamed engine runs residual networks only"); return MZX_ERR_INVALID; }
  net->rz_mode = mode ? 1 : 0;
  net->rz_waves = (mode == 2) ? 4 : 0;
  net->rb_force = (mode == 3 || mode == 4) ? 1 : 0;
  net->rb_no_towers = (mode == 4 || mode == 5) ? 1 : 0;
  return MZX_OK;
}

int64_t mzx_net_flops(const mzx_net* net, int32_t recurrent) {
  if (!net) return 0;
  int64_t macs = 0;
  for (const OpDesc& d : (recurrent ? net->prog_recurrent : net->prog_initial)) {
    switch (d.kind) {
      case OP_CONV3: macs += (int64_t)d.cout * d.hout * d.wout * d.cin * 9; break;
      case OP_CONVK: macs += (int64_t)d.cout * d.hout * d.wout * d.cin * d.ksize * d.ksize; break;
      case OP_CONV1: macs += (int64_t)d.cout * d.hin * d.cin; break;
      case OP_LINEAR: macs += (int64_t)d.out_features * d.w_stride; break;
      default: break;
    }
  }
  return 2 * macs;
}

int mzx_net_fused_schedule(const mzx_net* net, int32_t recurrent, int32_t* slot_of_op, int32_t cap) {
  if (!net || !slot_of_op) return 0;
  const RzProgram& R = recurrent ? net->rz.recurrent : net->rz.initial;
  const int n = (int)(recurrent ? net->prog_recurrent.size() : net->prog_initial.size());
  if (!net->rz.ok || !R.ok || cap < n) return 0;
  for (int k = 0; k < n; ++k) slot_of_op[k] = -1;
  for (int k = 0; k < R.n_ops; ++k) {
    int slot = 0;
    for (int q = 0; q < R.order[k]; ++q) slot += (int)((R.ops[q].sched >> 16) & 1u);
    slot_of_op[R.first + k] = slot;
  }
  return R.n_slots;
}

int mzx_net_num_operators(const mzx_net* net, int32_t recurrent) {
  if (!net) return 0;
  return (int)(recurrent ? net->prog_recurrent.size() : net->prog_initial.size());
}

static int check_net_call(const mzx_net* net, int32_t batch, int64_t workspace_floats) {
  if (!net) { set_error("null network handle"); return MZX_ERR_INVALID; }
  if (!net->d_flat) { set_error("network has no weights bound (call mzx_net_set_weights)"); return MZX_ERR_INVALID; }
  if (batch < 1) { set_error("batch must be >= 1"); return MZX_ERR_INVALID; }
  if (workspace_floats < net_ws_per_sample(net) * (int64_t)batch) {
    set_error("workspace too small: %lld floats given, %lld needed", (long long)workspace_floats,
              (long long)(net_ws_per_sample(net) * (int64_t)batch));
    return MZX_ERR_WORKSPACE;
  }
  return MZX_OK;
}

int mzx_net_initial_inference(mzx_net* net, const float* d_observation, int32_t batch, float* d_value_logits,
                              float* d_reward_logits, float* d_policy_logits, float* d_hidden, float* d_workspace,
                              int64_t workspace_floats, void* stream) {
  int rc = check_net_call(net, batch, workspace_floats);
  if (rc) return rc;
  if (!d_observation || !d_value_logits || !d_policy_logits || !d_hidden) { set_error("null buffer"); return MZX_ERR_INVALID; }
  NetBuffers nb;
  nb.in = d_observation; nb.action = nullptr; nb.hidden = d_hidden; nb.value = d_value_logits;
  nb.reward = nullptr; nb.policy = d_policy_logits; nb.workspace = d_workspace;
  rc = run_network(net, false, nb, batch, (stream_t)stream);
  if (rc) return rc;
  if (d_reward_logits) {
    RewardFillOp f;
    f.y = d_reward_logits; f.batch = batch; f.full_support = net->full_support;
    MZX_TRY_LAUNCH(launch<256>(f, (stream_t)stream));
  }
  return MZX_OK;
}

int mzx_net_recurrent_inference(mzx_net* net, const float* d_hidden, const int32_t* d_action, int32_t batch,
                                float* d_value_logits, float* d_reward_logits, float* d_policy_logits,
                                float* d_next_hidden, float* d_workspace, int64_t workspace_floats, void* stream) {
  int rc = check_net_call(net, batch, workspace_floats);
  if (rc) return rc;
  if (!d_hidden || !d_action || !d_value_logits || !d_reward_logits || !d_policy_logits || !d_next_hidden) {
    set_error("null buffer");
    return MZX_ERR_INVALID;
  }
  NetBuffers nb;
  nb.in = d_hidden; nb.action = d_action; nb.hidden = d_next_hidden; nb.value = d_value_logits;
  nb.reward = d_reward_logits; nb.policy = d_policy_logits; nb.workspace = d_workspace;
  return run_network(net, true, nb, batch, (stream_t)stream);
}

int mzx_net_debug_prefix(mzx_net* net, int32_t recurrent, int32_t fused, int32_t n_ops, const float* d_input,
                         const int32_t* d_action, int32_t batch, float* d_out, int64_t out_floats, float* d_scratch,
                         int64_t scratch_floats, float* d_workspace, int64_t workspace_floats, void* stream) {
  int rc = check_net_call(net, batch, workspace_floats);
  if (rc) return rc;
  const int64_t need = (net->hidden_size + 2 * net->full_support + net->cfg.action_space_size) * (int64_t)batch;
  if (!d_input || !d_out || !d_scratch || scratch_floats < need) { set_error("debug_prefix: missing / short buffer (%lld scratch floats)", (long long)need); return MZX_ERR_WORKSPACE; }
  NetBuffers nb;
  nb.in = d_input; nb.action = d_action; nb.workspace = d_workspace;
  nb.hidden = d_scratch;
  nb.value = nb.hidden + net->hidden_size * batch;
  nb.reward = nb.value + (int64_t)net->full_support * batch;
  nb.policy = nb.reward + (int64_t)net->full_support * batch;
  return run_network_prefix(net, recurrent != 0, fused, n_ops, nb, batch, d_out, out_floats, (stream_t)stream);
}

// ----------------------------------------------------------------- search

int mzx_search_create(const mzx_search_config* cfg, mzx_net* net, mzx_search** out) {
  if (!cfg || !out) { set_error("mzx_search_create: null argument"); return MZX_ERR_INVALID; }
  if (cfg->num_trees < 1 || cfg->num_simulations < 0 || cfg->action_space_size < 1) {
    set_error("num_trees/num_simulations/action_space_size out of range");
    return MZX_ERR_INVALID;
  }
  if (cfg->num_players != 1 && cfg->num_players != 2) {
    // self_play.py:429-430
    set_error("More than two player mode not implemented.");
    return MZX_ERR_INVALID;
  }
  if (!cfg->h_pb_c_table || !cfg->h_sqrt_table) { set_error("pb_c / sqrt tables are required"); return MZX_ERR_INVALID; }
  if (net && net->cfg.action_space_size != cfg->action_space_size) { set_error("network/search action space mismatch"); return MZX_ERR_INVALID; }
  if (net && net->cfg.support_size != cfg->support_size) { set_error("network/search support size mismatch"); return MZX_ERR_INVALID; }
  mzx_search* s = new (std::nothrow) mzx_search();
  if (!s) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  s->cfg = *cfg;
  s->net = net;
  const int n = cfg->num_simulations + 2;
  s->h_pbc.assign(cfg->h_pb_c_table, cfg->h_pb_c_table + (n - 1));
  s->h_sqrt.assign(cfg->h_sqrt_table, cfg->h_sqrt_table + (n - 1));
  s->h_pbc.push_back(0.0);
  s->h_sqrt.push_back(0.0);
  s->cfg.h_pb_c_table = nullptr;
  s->cfg.h_sqrt_table = nullptr;
  search_plan(s);
  if (int rc = upload_tables(s)) { mzx_search_destroy(s); return rc; }
#ifndef MZX_HOSTCHECK
  // 1: fully connected whole-search kernel, 2: residual whole-search kernels, 3: row-per-tree kernels around a
  // network that runs layer by layer on the streamed MFMA engine
  s->fused_ok = fc2_plan(s).ok ? 1 : (rz_search_supported(s) ? 2 : ((net && net->rb.ok && net->rb.recurrent.ok && row_search_supported(s->p)) ? 3 : 0));
#endif
  s->mode = s->fused_ok ? 1 : 0;
  *out = s;
  return MZX_OK;
}

void mzx_search_destroy(mzx_search* s) {
  if (s && s->d_tables) device_free(s->d_tables);
#ifndef MZX_HOSTCHECK
  if (s && s->side_stream) {      // the row-per-tree path's second stream (joined at the end of every run)
    (void)hipStreamSynchronize((hipStream_t)s->side_stream);
    if (s->ev_fork) (void)hipEventDestroy((hipEvent_t)s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy((hipEvent_t)s->ev_join);
    (void)hipStreamDestroy((hipStream_t)s->side_stream);
  }
#endif
  delete s;
}

int64_t mzx_search_arena_bytes(const mzx_search* s) { return s ? s->arena_bytes : 0; }

int mzx_search_fused_supported(const mzx_search* s) { return s ? s->fused_ok : 0; }

const char* mzx_search_kernel_name(const mzx_search* s) { return s ? s->last_kernel : ""; }

int mzx_search_arena_offsets(const mzx_search* s, int64_t out[8]) {
  if (!s || !out) { set_error("null argument"); return MZX_ERR_INVALID; }
  out[0] = s->off_tables; out[1] = s->off_trees; out[2] = s->off_hidden; out[3] = s->off_ws;
  out[4] = s->L.tree_bytes; out[5] = s->ws_floats * 4; out[6] = s->arena_bytes; out[7] = 0;
  return MZX_OK;
}

int mzx_tuning_set(const char* name, int32_t value) {
  const int k = tuning_find(name);
  if (k < 0) { set_error("unknown tuning entry '%s'", name ? name : "(null)"); return MZX_ERR_INVALID; }
  TuningEntry& e = tuning_table()[k];
  if (value < e.lo || value > e.hi) { set_error("tuning entry '%s' takes %d .. %d", e.name, e.lo, e.hi); return MZX_ERR_INVALID; }
  e.value = value;
  return MZX_OK;
}

int mzx_tuning_get(const char* name, int32_t* value, int32_t* dflt) {
  const int k = tuning_find(name);
  if (k < 0) { set_error("unknown tuning entry '%s'", name ? name : "(null)"); return MZX_ERR_INVALID; }
  if (value) *value = tuning_table()[k].value;
  if (dflt) *dflt = tuning_table()[k].dflt;
  return MZX_OK;
}

const char* mzx_tuning_name(int32_t index) { return (index >= 0 && index < TUNE_COUNT) ? tuning_table()[index].name : nullptr; }
const char* mzx_tuning_help(int32_t index) { return (index >= 0 && index < TUNE_COUNT) ? tuning_table()[index].what : nullptr; }

// The one route decision of a search on this handle, for its three entries: mzx_search_run (FRESH), mzx_search_run_from_roots
// (OVERRIDE) and mzx_search_run_continued (CONTINUED) launch what it names (search_simulate), mzx_search_route reports the
// FRESH one.  A handle with spare node capacity (mzx_search_set_capacity) takes only kernels that leave every node's hidden
// state in the arena for mzx_search_advance and that take carried trees: fc2_search_kernel where its LDS plan fits the
// capacity (it exports every search), rt_search_kernel and the streamed row route (the node store), or the per-operator path.
// The LDS-resident residual kernels (rz_*) and the first-generation fully connected kernel (flag 16) do not; such a handle
// runs the per-operator path instead.
// A CONTINUED search takes the route of a FRESH one.  An OVERRIDE search does not in every case: the rules marked "from roots"
// keep what mzx_search_run_from_roots chose while it had an if-chain of its own (tests/test_gpu_route_table.py pins them);
// whether such a search should follow the fresh route is a decision to take on purpose, not made here.
static SearchChoice search_choice(const mzx_search* s, SearchStart::Kind kind) {
  SearchChoice c;
#ifndef MZX_HOSTCHECK
  if (!s->net || !(s->mode & 1)) return c;
  const bool spare = s->max_nodes > 0;
  const bool from_roots = kind == SearchStart::OVERRIDE;
  if (s->fused_ok == 1 && !spare) {
    if (!(s->mode & 16)) { c.path = PATH_FC2; return c; }
    // from roots: the first-generation kernel (flag 16, experiment builds) takes no given roots -- the per-operator path
    if (!from_roots) { c.path = PATH_FUSED_FC; return c; }
  }
  // from roots: never fc2_search_kernel on a spare-capacity handle -- the per-operator path
  if (s->fused_ok == 1 && spare && !from_roots && !(s->mode & 16) && fc2_fits(s)) { c.path = PATH_FC2; return c; }
  // from roots: a spare-capacity handle skips the wide-network rule -- the row route below only when the network handle's own
  // mode selects the streamed engine, else the per-operator path (the LDS-resident engine's arithmetic)
  if (s->fused_ok == 2 && rz_enabled(s->net, true) && !(from_roots && spare)) {
    // a wide network: the tower arithmetic at every shard size (wide_search_route, mzx_row_search.h) -- all simulations in
    // one launch of rt_search_kernel, or the trunks as towers between the row-per-tree kernels
    const int route = wide_search_route(s);
    if (route != ROUTE_RZ) { c.path = route == ROUTE_RT ? PATH_RT : PATH_ROWS; c.force_streamed = true; return c; }
    if (!spare) { c.path = PATH_RZ; return c; }
  }
  if (rb_enabled(s->net, true) && row_search_supported(s->p)) {
    // from roots: launch by launch on a spare-capacity handle, also where the fresh search takes rt_search_kernel
    c.path = !(from_roots && spare) && streamed_whole_search(s) ? PATH_RT : PATH_ROWS;
  }
#else
  (void)s; (void)kind;
#endif
  return c;
}

static void search_route_of(const mzx_search* s, int32_t out[8]) {
  for (int k = 0; k < 8; ++k) out[k] = 0;
#ifndef MZX_HOSTCHECK
  static const int32_t code[] = {0, 1, 2, 3, 4, 4};   // indexed by SearchPath
  out[0] = code[search_choice(s, SearchStart::FRESH).path];
  if (out[0] == 3) rt_search_shape(s, out + 1);      // out[1 .. 6]
  if (out[0] == 2) {
    const int first = rb_split_first(s->net, s->p.num_trees, tune(TUNE_ROW_SPLIT_MIN));
    out[6] = first > 0 ? first : s->p.num_trees;
    out[7] = first > 0 ? s->p.num_trees - first : 0;
  }
#endif
}

int mzx_search_route(const mzx_search* s, int32_t out[8]) {
  if (!s || !out) { set_error("null argument"); return MZX_ERR_INVALID; }
  search_route_of(s, out);
  return MZX_OK;
}

int mzx_net_search_route(const mzx_net* net, int32_t num_trees, int32_t num_simulations, int32_t out[8]) {
  if (!net || !out || num_trees < 1 || num_simulations < 0) { set_error("null argument / sizes out of range"); return MZX_ERR_INVALID; }
  // a search descriptor without device tables: the planner only reads sizes (host-side, no GPU)
  mzx_search tmp;
  memset(&tmp.cfg, 0, sizeof(tmp.cfg));
  tmp.cfg.num_trees = num_trees; tmp.cfg.num_simulations = num_simulations;
  tmp.cfg.action_space_size = net->cfg.action_space_size; tmp.cfg.support_size = net->cfg.support_size;
  tmp.cfg.num_players = 1; tmp.cfg.tape_words = 16; tmp.cfg.discount = 1.0; tmp.cfg.root_exploration_fraction = 0.25;
  tmp.net = const_cast<mzx_net*>(net);
  search_plan(&tmp);
#ifndef MZX_HOSTCHECK
  tmp.fused_ok = fc2_plan(&tmp).ok ? 1 : (rz_search_supported(&tmp) ? 2 : ((net->rb.ok && net->rb.recurrent.ok && row_search_supported(tmp.p)) ? 3 : 0));
#endif
  tmp.mode = tmp.fused_ok ? 1 : 0;
  search_route_of(&tmp, out);
  return MZX_OK;
}

int mzx_search_set_mode(mzx_search* s, int32_t mode) {
  if (!s) { set_error("null search handle"); return MZX_ERR_INVALID; }
  if (mode < 0 || mode > 31) { set_error("mode is a 5-bit flag set"); return MZX_ERR_INVALID; }
#if !defined(MZX_HOSTCHECK) && defined(MZX_EXPERIMENT)
  if ((mode & 16) && !(s->fused_ok == 1 && fused_fc_supported(s))) { set_error("flag 16 selects the first-generation fully connected kernel"); return MZX_ERR_INVALID; }
#else
  if (mode & 16) { set_error("flag 16 (the first-generation fully connected kernel) needs an instrumented build (-DMZX_EXPERIMENT)"); return MZX_ERR_INVALID; }
#endif
  if ((mode & 1) && !s->fused_ok) { set_error("fused search kernel does not support this configuration"); return MZX_ERR_INVALID; }
  s->mode = mode;
  return MZX_OK;
}

static int check_search_call(const mzx_search* s, const void* d_arena, int64_t arena_bytes, bool need_net) {
  if (!s || !d_arena) { set_error("null search handle / arena"); return MZX_ERR_INVALID; }
  if (arena_bytes >= 0 && arena_bytes < s->arena_bytes) {
    set_error("arena too small: %lld bytes given, %lld needed", (long long)arena_bytes, (long long)s->arena_bytes);
    return MZX_ERR_WORKSPACE;
  }
  if (need_net && (!s->net || !s->net->d_flat)) { set_error("search needs a network with bound weights"); return MZX_ERR_INVALID; }
  if (s->device >= 0 && current_device() != s->device) {   // its tables (and the caller's arena) live on that device
    set_error("search handle was created on device %d, the current device is %d", s->device, current_device());
    return MZX_ERR_INVALID;
  }
  return MZX_OK;
}

// The simulations of a search whose roots arrive as `start` says, on the route search_choice names.  The one place that
// records the kernel (the drivers refine it where they decide: rz_search_run among its three kernels, search_run_rows when
// it runs two half-shards) and whether the arena now holds every node's hidden state (mzx_search_advance).
static int search_simulate(mzx_search* s, const mzx_search_io* io, void* d_arena, stream_t stream, const SearchStart& start) {
  const SearchChoice c = search_choice(s, start.kind);
  int rc = MZX_OK;
  switch (c.path) {
#ifndef MZX_HOSTCHECK
    case PATH_FUSED_FC:
      s->last_kernel = KERNEL_FUSED_FC;
      rc = fused_fc_run(s, io, d_arena, stream, start);
      break;
    case PATH_FC2:
      s->last_kernel = KERNEL_FC2;
      rc = fc2_run(s, io, d_arena, stream, start);
      break;
    case PATH_RZ:
      rc = rz_search_run(s, io, d_arena, stream, start);
      break;
    case PATH_ROWS:
    case PATH_RT:
      s->last_kernel = c.path == PATH_RT ? KERNEL_RT : KERNEL_ROWS;
      rc = search_run_rows(s, io, d_arena, stream, start, c.force_streamed, c.path == PATH_RT);
      break;
#endif
    default:
      // from roots: the plain name, also where the network runs on the streamed engine
      s->last_kernel = start.kind != SearchStart::OVERRIDE && rb_enabled(s->net, true) ? KERNEL_GENERIC_STREAMED : KERNEL_GENERIC;
      rc = search_run_generic(s, io, d_arena, stream, start);
      break;
  }
  // the per-operator path, the row route and rt_search_kernel keep every node's hidden state in the arena's store;
  // fc2_search_kernel exports it for handles with spare capacity; the other whole-search kernels keep it in LDS
  const bool leaves_hidden = c.path == PATH_GENERIC || c.path == PATH_ROWS || c.path == PATH_RT || (c.path == PATH_FC2 && s->max_nodes > 0);
  if (!rc && leaves_hidden) s->hidden_arena = d_arena;
  return rc;
}

int mzx_search_run(mzx_search* s, const mzx_search_io* io, void* d_arena, int64_t arena_bytes, void* stream) {
  int rc = check_search_call(s, d_arena, arena_bytes, true);
  if (rc) return rc;
  if (!io || !io->d_observation || !io->d_legal_actions || !io->d_to_play || !io->d_tape || !io->d_visit_counts ||
      !io->d_root_value || !io->d_info) {
    set_error("mzx_search_run: missing io buffer");
    return MZX_ERR_INVALID;
  }
  s->hidden_arena = s->carried_arena = nullptr;
  return search_simulate(s, io, d_arena, (stream_t)stream, SearchStart{});
}

int mzx_search_run_from_roots(mzx_search* s, const mzx_search_io* io, const float* d_root_hidden,
                              const double* d_root_priors, const double* d_root_reward, void* d_arena,
                              int64_t arena_bytes, void* stream) {
  int rc = check_search_call(s, d_arena, arena_bytes, true);
  if (rc) return rc;
  if (!io || !io->d_legal_actions || !io->d_to_play || !io->d_tape || !io->d_visit_counts || !io->d_root_value ||
      !io->d_info || !d_root_hidden || !d_root_priors || !d_root_reward) {
    set_error("mzx_search_run_from_roots: missing buffer");
    return MZX_ERR_INVALID;
  }
  s->hidden_arena = s->carried_arena = nullptr;
  return search_simulate(s, io, d_arena, (stream_t)stream, SearchStart{SearchStart::OVERRIDE, {d_root_hidden, d_root_priors, d_root_reward}});
}

int mzx_search_lockstep_begin(mzx_search* s, const mzx_search_io* io, const double* d_root_priors,
                              const double* d_root_reward, void* d_arena, int64_t arena_bytes, void* stream) {
  int rc = check_search_call(s, d_arena, arena_bytes, false);
  if (rc) return rc;
  if (!io || !io->d_legal_actions || !io->d_to_play || !d_root_priors) { set_error("lockstep_begin: missing buffer"); return MZX_ERR_INVALID; }
  s->carried_arena = nullptr;
  s->hidden_arena = s->net ? nullptr : d_arena;    // (a handle without a network carries trees alone)
  rc = ensure_tables(s);
  if (rc) return rc;
  const ArenaView v = arena_view(s, d_arena);
  RootInitOp ri;
  ri.arena = v.arena; ri.p = v.p; ri.value_logits = nullptr; ri.policy_logits = nullptr; ri.ext_priors = d_root_priors; ri.ext_root_reward = d_root_reward;
  ri.legal = io->d_legal_actions; ri.to_play = io->d_to_play; ri.noise = io->d_noise; ri.root_predicted_value = nullptr;
  MZX_TRY_LAUNCH(launch<64>(ri, (stream_t)stream));
  return MZX_OK;
}

int mzx_search_lockstep_select(mzx_search* s, const mzx_search_io* io, int32_t* d_parent, int32_t* d_action,
                               int32_t* d_leaf, void* d_arena, void* stream) {
  int rc = check_search_call(s, d_arena, -1, false);
  if (rc) return rc;
  if (!io || !io->d_tape || !d_parent || !d_action || !d_leaf) { set_error("lockstep_select: missing buffer"); return MZX_ERR_INVALID; }
  const ArenaView v = arena_view(s, d_arena);
  SelectOp sel;
  sel.arena = v.arena; sel.p = v.p; sel.tape = io->d_tape;
  sel.sel_parent = d_parent; sel.sel_action = d_action; sel.sel_leaf = d_leaf;
  MZX_TRY_LAUNCH(launch<64>(sel, (stream_t)stream));
  return MZX_OK;
}

int mzx_search_lockstep_apply(mzx_search* s, const double* d_value, const double* d_reward, const double* d_priors,
                              void* d_arena, void* stream) {
  int rc = check_search_call(s, d_arena, -1, false);
  if (rc) return rc;
  if (!d_value || !d_reward || !d_priors) { set_error("lockstep_apply: missing buffer"); return MZX_ERR_INVALID; }
  const ArenaView v = arena_view(s, d_arena);
  ExpandBackpropOp eb;
  eb.arena = v.arena; eb.p = v.p; eb.value_logits = nullptr; eb.reward_logits = nullptr; eb.policy_logits = nullptr;
  eb.ext_value = d_value; eb.ext_reward = d_reward; eb.ext_priors = d_priors;
  MZX_TRY_LAUNCH(launch<64>(eb, (stream_t)stream));
  return MZX_OK;
}

int mzx_search_finish(mzx_search* s, const mzx_search_io* io, void* d_arena, void* stream) {
  int rc = check_search_call(s, d_arena, -1, false);
  if (rc) return rc;
  if (!io || !io->d_visit_counts || !io->d_root_value || !io->d_info) { set_error("finish: missing buffer"); return MZX_ERR_INVALID; }
  return search_finish(s, io, d_arena, (stream_t)stream);
}

int mzx_search_dump(mzx_search* s, const mzx_tree_dump* dump, void* d_arena, void* stream) {
  int rc = check_search_call(s, d_arena, -1, false);
  if (rc) return rc;
  if (!dump) { set_error("dump: null"); return MZX_ERR_INVALID; }
  const ArenaView v = arena_view(s, d_arena);
  DumpOp op;
  op.arena = v.arena; op.p = v.p; op.d = *dump;
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------- continued searches (mzx_tree_carry.h)

int mzx_search_set_capacity(mzx_search* s, int32_t max_nodes, const double* h_pb_c_table, const double* h_sqrt_table) {
  if (!s || !h_pb_c_table || !h_sqrt_table) { set_error("mzx_search_set_capacity: null argument"); return MZX_ERR_INVALID; }
  if (max_nodes < s->cfg.num_simulations + 1 || max_nodes > (1 << 24)) {
    set_error("mzx_search_set_capacity: max_nodes %d must lie in num_simulations + 1 (%d) .. 2^24", max_nodes,
              s->cfg.num_simulations + 1);
    return MZX_ERR_INVALID;
  }
  std::vector<double> pbc(h_pb_c_table, h_pb_c_table + max_nodes), sq(h_sqrt_table, h_sqrt_table + max_nodes);
  pbc.push_back(0.0);
  sq.push_back(0.0);
  double* old = s->d_tables;
  const int32_t old_nodes = s->max_nodes;
  s->h_pbc.swap(pbc);
  s->h_sqrt.swap(sq);
  s->max_nodes = max_nodes;
  search_plan(s);
  s->d_tables = nullptr;
  if (int rc = upload_tables(s)) {       // keep the handle as it was
    s->h_pbc.swap(pbc);
    s->h_sqrt.swap(sq);
    s->max_nodes = old_nodes;
    search_plan(s);
    s->d_tables = old;
    return rc;
  }
  if (old) device_free(old);
  s->hidden_arena = s->carried_arena = nullptr;
  s->rt_plan_key[0] = -1;
  return MZX_OK;
}

int mzx_search_advance(mzx_search* s, const int32_t* d_actions, void* d_src_arena, void* d_dst_arena, void* stream) {
  int rc = check_search_call(s, d_dst_arena, -1, false);
  if (rc) return rc;
  if (!d_actions || !d_src_arena) { set_error("mzx_search_advance: null argument"); return MZX_ERR_INVALID; }
  if (d_src_arena == d_dst_arena) { set_error("mzx_search_advance: the source and destination arenas must differ"); return MZX_ERR_INVALID; }
  if (s->off_carry < 0) { set_error("mzx_search_advance: the handle has no node capacity for carried trees (mzx_search_set_capacity)"); return MZX_ERR_INVALID; }
  if (!s->hidden_arena || s->hidden_arena != d_src_arena) {
    set_error("mzx_search_advance: the last search of this handle did not leave every node's hidden state in d_src_arena "
              "(route: %s)", s->last_kernel[0] ? s->last_kernel : "none yet");
    return MZX_ERR_INVALID;
  }
  const ArenaView src = arena_view(s, d_src_arena), dst = arena_view(s, d_dst_arena);
  TreeAdvanceArgs a;
  a.p = src.p; a.L = s->L;
  a.src_trees = src.arena.trees; a.dst_trees = dst.arena.trees;
  a.src_hidden = src.arena.hidden; a.dst_hidden = dst.arena.hidden;
  a.scratch = (int32_t*)((char*)d_dst_arena + s->off_rowpath);     // 2 N + 2 ints per tree: the row kernels' path store
  a.actions = d_actions;
  a.carry = (int32_t*)((char*)d_dst_arena + s->off_carry);
  MZX_TRY_LAUNCH(tree_advance_launch(a, (stream_t)stream));
  s->hidden_arena = s->carried_arena = d_dst_arena;
  return MZX_OK;
}

int mzx_search_load(mzx_search* s, const mzx_tree_load* h, void* d_arena, void* stream) {
  int rc = check_search_call(s, d_arena, -1, false);
  if (rc) return rc;
  if (!h || !h->h_visit || !h->h_value_sum || !h->h_reward || !h->h_to_play || !h->h_parent || !h->h_child || !h->h_prior ||
      !h->h_n_nodes || !h->h_root_actions || (s->p.hidden_size > 0 && !h->h_hidden)) {
    set_error("mzx_search_load: missing array");
    return MZX_ERR_INVALID;
  }
  if (s->off_carry < 0) { set_error("mzx_search_load: the handle has no node capacity for carried trees (mzx_search_set_capacity)"); return MZX_ERR_INVALID; }
  const int B = s->p.num_trees, N = s->p.num_nodes, M = h->max_nodes;
  const int64_t Hf = s->p.hidden_size;
  if (M < 1) { set_error("mzx_search_load: max_nodes must be positive"); return MZX_ERR_INVALID; }
  std::vector<char> image((size_t)s->L.tree_bytes * B);
  std::vector<int32_t> carry((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    const int nn = h->h_n_nodes[b];
    if (nn < 1 || nn > M || nn + s->p.num_sims + 1 > N) {
      set_error("mzx_search_load: tree %d has %d nodes; %d node slots given, capacity %d for %d more simulations", b, nn, M, N,
                s->p.num_sims);
      return MZX_ERR_INVALID;
    }
    TreeRef t;
    t.base = image.data() + (size_t)b * s->L.tree_bytes;
    t.L = s->L;
    if (pack_loaded_tree(t, s->p, *h, b)) {
      set_error("mzx_search_load: tree %d is not a canonical-order tree this handle can continue (parents before children, "
                "child links matching parents, visit counts + num_simulations below the capacity)", b);
      return MZX_ERR_INVALID;
    }
    carry[2 * b] = nn;
    carry[2 * b + 1] = t.to_play(0);
  }
  const ArenaView v = arena_view(s, d_arena);
  const stream_t st = (stream_t)stream;
  MZX_TRY_LAUNCH(copy_h2d(v.arena.trees, image.data(), image.size(), st));
  MZX_TRY_LAUNCH(copy_h2d((char*)d_arena + s->off_carry, carry.data(), carry.size() * sizeof(int32_t), st));
  if (Hf > 0) {
    for (int b = 0; b < B; ++b)
      MZX_TRY_LAUNCH(copy_h2d(v.arena.hidden + (int64_t)b * N * Hf, h->h_hidden + (int64_t)b * M * Hf,
                              sizeof(float) * Hf * h->h_n_nodes[b], st));
  }
  MZX_TRY_LAUNCH(stream_sync(st));      // (the host image is released on return)
  s->hidden_arena = s->carried_arena = d_arena;
  return MZX_OK;
}

int mzx_search_run_continued(mzx_search* s, const mzx_search_io* io, void* d_arena, int64_t arena_bytes, void* stream) {
  int rc = check_search_call(s, d_arena, arena_bytes, false);
  if (rc) return rc;
  const bool with_net = s->net != nullptr;
  if (with_net && !s->net->d_flat) { set_error("search needs a network with bound weights"); return MZX_ERR_INVALID; }
  if (!io || !io->d_to_play || (with_net && (!io->d_tape || !io->d_visit_counts || !io->d_root_value || !io->d_info))) {
    set_error("mzx_search_run_continued: missing io buffer");
    return MZX_ERR_INVALID;
  }
  if (!s->carried_arena || s->carried_arena != d_arena) {
    set_error("mzx_search_run_continued: d_arena holds no carried trees (mzx_search_advance / mzx_search_load of this handle "
              "put them there; a search call since then used them up)");
    return MZX_ERR_INVALID;
  }
  const int B = s->p.num_trees, N = s->p.num_nodes, S = s->p.num_sims;
  const stream_t st = (stream_t)stream;
  std::vector<int32_t> carry((size_t)2 * B), tp((size_t)B);
  MZX_TRY_LAUNCH(copy_d2h(carry.data(), (char*)d_arena + s->off_carry, carry.size() * sizeof(int32_t), st));
  MZX_TRY_LAUNCH(copy_d2h(tp.data(), io->d_to_play, tp.size() * sizeof(int32_t), st));
  MZX_TRY_LAUNCH(stream_sync(st));
  for (int b = 0; b < B; ++b) {
    if (carry[2 * b] + S + 1 > N) {
      set_error("mzx_search_run_continued: tree %d carries %d nodes; with %d simulations it needs %d node slots, the handle has %d "
                "(mzx_search_set_capacity)", b, carry[2 * b], S, carry[2 * b] + S + 1, N);
      return MZX_ERR_INVALID;
    }
    if (carry[2 * b + 1] != tp[b]) {
      set_error("mzx_search_run_continued: to_play %d of tree %d differs from its carried root's to_play %d", tp[b], b, carry[2 * b + 1]);
      return MZX_ERR_INVALID;
    }
  }
  const ArenaView v = arena_view(s, d_arena);
  ContinueRootOp cr;
  cr.arena = v.arena; cr.p = v.p; cr.noise = io->d_noise; cr.root_predicted_value = io->d_root_predicted_value;
  MZX_TRY_LAUNCH(launch<64>(cr, st));
  s->carried_arena = nullptr;
  s->hidden_arena = d_arena;
  if (!with_net) return MZX_OK;     // lock-step handle: the caller drives the simulations
  s->hidden_arena = nullptr;
  // the route of a fresh search on this handle (search_choice): fc2_search_kernel / rt_search_kernel import the carried
  // trees, the streamed row route and the per-operator path walk them in the arena
  return search_simulate(s, io, d_arena, st, SearchStart{SearchStart::CONTINUED});
}

// ------------------------------------------------------- observation pipeline

static bool obs_layout_ok(const mzx_obs_layout* L) {
  return L && L->channels >= 1 && L->height >= 1 && L->width >= 1 && L->stacked_observations >= 0 &&
         L->action_space_size >= 1 && L->num_games >= 1 && L->ring >= 1 &&
         (int64_t)L->channels * (L->stacked_observations + 1) + L->stacked_observations < (1 << 20);
}

int64_t mzx_obs_stacked_floats(const mzx_obs_layout* L) {
  if (!obs_layout_ok(L)) return 0;
  return ((int64_t)L->channels * (L->stacked_observations + 1) + L->stacked_observations) * L->height * L->width;
}

extern "C++" {
template <int VEC>
static int obs_stack_launch(const mzx_obs_layout* L, const float* d_frames, const int32_t* d_actions,
                            const int32_t* d_game, const int32_t* d_time, int32_t time0, int32_t n_out, float* d_out,
                            stream_t stream) {
  ObsStackOp<VEC> op;
  op.frames = d_frames; op.actions = d_actions; op.game = d_game; op.time = d_time; op.out = d_out;
  op.time0 = time0; op.C = L->channels; op.hwv = L->height * L->width / VEC; op.k = L->stacked_observations;
  op.A = L->action_space_size; op.G = L->num_games; op.ring = L->ring; op.n_out = n_out;
  op.c_out = L->channels * (L->stacked_observations + 1) + L->stacked_observations;
  op.pieces = (op.hwv + 64 * ObsStackOp<VEC>::UNROLL - 1) / (64 * ObsStackOp<VEC>::UNROLL);
  if ((int64_t)n_out * op.c_out * op.pieces >= (int64_t)1 << 26) {   // 32-bit group index; split the call
    set_error("obs_stack: %d samples x %d planes exceed one launch; stack in smaller batches", n_out, op.c_out);
    return MZX_ERR_INVALID;
  }
  MZX_TRY_LAUNCH(launch<256>(op, stream));
  return MZX_OK;
}
}  // extern "C++"

int mzx_obs_stack(const mzx_obs_layout* L, const float* d_frames, const int32_t* d_actions, const int32_t* d_game,
                  const int32_t* d_time, int32_t time0, int32_t n_out, float* d_out, void* stream) {
  if (!obs_layout_ok(L)) { set_error("obs_stack: invalid layout"); return MZX_ERR_INVALID; }
  if (n_out < 0 || time0 < 0) { set_error("obs_stack: negative n_out / time0"); return MZX_ERR_INVALID; }
  if (n_out == 0) return MZX_OK;
  if (!d_frames || !d_out || (L->stacked_observations > 0 && !d_actions)) { set_error("obs_stack: missing buffer"); return MZX_ERR_INVALID; }
  if (!d_time && L->ring < L->stacked_observations + 1 && (int64_t)time0 + (n_out - 1) / L->num_games >= L->ring) {
    set_error("obs_stack: ring %d cannot hold %d stacked observations at index %d", L->ring, L->stacked_observations, time0);
    return MZX_ERR_INVALID;
  }
  const bool vec = (L->height * L->width) % 4 == 0 && ((uintptr_t)d_frames % 16) == 0 && ((uintptr_t)d_out % 16) == 0;
  return vec ? obs_stack_launch<4>(L, d_frames, d_actions, d_game, d_time, time0, n_out, d_out, (stream_t)stream)
             : obs_stack_launch<1>(L, d_frames, d_actions, d_game, d_time, time0, n_out, d_out, (stream_t)stream);
}

int mzx_support_to_scalar(const float* d_logits, int32_t rows, int32_t support_size, float* d_out, void* stream) {
  if (rows < 0 || support_size < 0) { set_error("support_to_scalar: negative argument"); return MZX_ERR_INVALID; }
  if (rows == 0) return MZX_OK;
  if (!d_logits || !d_out) { set_error("support_to_scalar: missing buffer"); return MZX_ERR_INVALID; }
  SupportToScalarOp op;
  op.logits = d_logits; op.out = d_out; op.rows = rows; op.support_size = support_size;
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------------- random streams

int mzx_rng_create(int32_t num_streams, mzx_rng** out) {
  if (num_streams < 1 || !out) { set_error("mzx_rng_create: invalid argument"); return MZX_ERR_INVALID; }
  mzx_rng* r = new (std::nothrow) mzx_rng();
  if (!r) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  r->streams.resize(num_streams);
  for (int32_t i = 0; i < num_streams; ++i) r->streams[i].seed((uint32_t)i);
  *out = r;
  return MZX_OK;
}

void mzx_rng_destroy(mzx_rng* r) { delete r; }

int mzx_rng_seed(mzx_rng* r, int32_t first, int32_t count, const uint32_t* seeds) {
  if (!r || !seeds || first < 0 || count < 0 || first + count > (int32_t)r->streams.size()) { set_error("mzx_rng_seed: range"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k) r->streams[first + k].seed(seeds[k]);
  return MZX_OK;
}

int mzx_rng_get_state(const mzx_rng* r, int32_t i, uint32_t* key, int32_t* pos, int32_t* has_gauss, double* gauss) {
  if (!r || i < 0 || i >= (int32_t)r->streams.size() || !key || !pos || !has_gauss || !gauss) { set_error("mzx_rng_get_state: argument"); return MZX_ERR_INVALID; }
  const Mt19937& m = r->streams[i];
  memcpy(key, m.key, sizeof(m.key));
  *pos = m.pos; *has_gauss = m.has_gauss; *gauss = m.gauss;
  return MZX_OK;
}

int mzx_rng_set_state(mzx_rng* r, int32_t i, const uint32_t* key, int32_t pos, int32_t has_gauss, double gauss) {
  if (!r || i < 0 || i >= (int32_t)r->streams.size() || !key || pos < 0 || pos > 624) { set_error("mzx_rng_set_state: argument"); return MZX_ERR_INVALID; }
  Mt19937& m = r->streams[i];
  memcpy(m.key, key, sizeof(m.key));
  m.pos = pos; m.has_gauss = has_gauss ? 1 : 0; m.gauss = gauss;
  return MZX_OK;
}

int mzx_rng_root_draws(mzx_rng* r, const int32_t* idx, int32_t count, double alpha, const int32_t* n_legal,
                       int32_t action_space_size, double* noise, int32_t tape_words, uint32_t* tape, int32_t n_threads) {
  int rc = rng_check(r, idx, count);
  if (rc) return rc;
  if ((noise && !n_legal) || action_space_size < 1 || tape_words < 0 || (tape_words > 0 && !tape)) { set_error("mzx_rng_root_draws: argument"); return MZX_ERR_INVALID; }
  if (noise)
    for (int32_t k = 0; k < count; ++k)
      if (n_legal[k] < 1 || n_legal[k] > action_space_size) { set_error("n_legal[%d] = %d out of range", k, n_legal[k]); return MZX_ERR_INVALID; }
  rng_parallel(r, count, n_threads, [=](int lo, int hi) {
    for (int k = lo; k < hi; ++k) {
      rng_prefetch_next(r, idx, k, hi);
      Mt19937& m = r->streams[idx[k]];
      if (noise) dirichlet_row(m, alpha, n_legal[k], action_space_size, noise + (size_t)k * action_space_size);
      if (tape_words > 0) m.peek(tape_words, tape + (size_t)k * tape_words);   // generator state untouched
    }
  });
  return MZX_OK;
}

int mzx_rng_advance(mzx_rng* r, const int32_t* idx, int32_t count, const int32_t* words) {
  int rc = rng_check(r, idx, count);
  if (rc) return rc;
  if (count > 0 && !words) { set_error("mzx_rng_advance: null"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k) {
    Mt19937& m = r->streams[idx[k]];
    for (int32_t j = 0; j < words[k]; ++j) m.next32();
  }
  return MZX_OK;
}

int mzx_rng_random_sample(mzx_rng* r, const int32_t* idx, int32_t count, double* out) {
  int rc = rng_check(r, idx, count);
  if (rc) return rc;
  if (count > 0 && !out) { set_error("mzx_rng_random_sample: null"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k) out[k] = r->streams[idx[k]].next_double();
  return MZX_OK;
}

int mzx_rng_randint(mzx_rng* r, const int32_t* idx, int32_t count, const int32_t* n, int32_t* out) {
  int rc = rng_check(r, idx, count);
  if (rc) return rc;
  if (count > 0 && (!n || !out)) { set_error("mzx_rng_randint: null"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k) {
    if (n[k] < 1) { set_error("randint(0, %d): empty range", n[k]); return MZX_ERR_INVALID; }
    out[k] = (int32_t)r->streams[idx[k]].bounded((uint32_t)n[k]);
  }
  return MZX_OK;
}

int mzx_rng_choice_weighted(mzx_rng* r, const int32_t* idx, int32_t count, const double* weights,
                            int32_t row_stride, const int32_t* n, int32_t* out) {
  int rc = rng_check(r, idx, count);
  if (rc) return rc;
  if (count > 0 && (!weights || !n || !out)) { set_error("mzx_rng_choice_weighted: null"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k)
    if (n[k] < 1 || n[k] > row_stride || n[k] > 4096) { set_error("choice: row %d has %d candidates (stride %d)", k, n[k], row_stride); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < count; ++k) {
    const double* w = weights + (size_t)k * row_stride;
    const int m = n[k];
    double total = 0.0;                       // Python's sum(dist): 0 + d0 + d1 + ...
    for (int j = 0; j < m; ++j) total = total + w[j];
    double cdf[4096];
    double acc = 0.0;                         // ndarray.cumsum of p = dist / total
    for (int j = 0; j < m; ++j) { acc = acc + w[j] / total; cdf[j] = acc; }
    const double last = cdf[m - 1];
    const double u = r->streams[idx[k]].next_double();
    int pos = 0;                              // searchsorted(u, side="right") on cdf / cdf[-1]
    for (int j = 0; j < m; ++j) pos += (cdf[j] / last <= u) ? 1 : 0;
    out[k] = pos;
  }
  return MZX_OK;
}

// ------------------------------------------------------------- a self-play move of a shard behind two calls (mzx_selfplay.h)

int mzx_selfplay_search(mzx_search* s, mzx_rng* r, const mzx_move* m, int32_t* n_legal, void* d_arena,
                        int64_t arena_bytes, void* stream) {
  const char* who = "mzx_selfplay_search";
  int rc = move_check(r, m);
  if (rc) return rc;
  if (!s) { set_error("%s: missing buffer", who); return MZX_ERR_INVALID; }
  rc = move_stage(m, n_legal, who, true);
  if (rc) return rc;
  const int B = m->num_games, A = m->action_space_size, W = m->tape_words;
  double* h_noise = move_in_host(m, m->io.d_noise);
  uint32_t* h_tape = move_in_host(m, m->io.d_tape);
  const double alpha = m->dirichlet_alpha;
  const int32_t* idx = m->streams;
  rng_parallel(r, B, m->num_threads, [=](int lo, int hi) {
    for (int k = lo; k < hi; ++k) {
      rng_prefetch_next(r, idx, k, hi);
      Mt19937& g = r->streams[idx[k]];
      if (h_noise) dirichlet_row(g, alpha, n_legal[k], A, h_noise + (size_t)k * A);
      if (W > 0) g.peek(W, h_tape + (size_t)k * W);       // generator state untouched
    }
  });
  rc = move_upload(m, stream);
  if (rc) return rc;
  // (instrumented builds only, -DMZX_EXPERIMENT: the host envelope of a move timed without the search)
  if (!exp_int("MZX_MOVE_NO_SEARCH", 0)) {
    rc = mzx_search_run(s, &m->io, d_arena, arena_bytes, stream);
    if (rc) return rc;
  }
  return move_finish(m, stream);
}

int mzx_selfplay_select(mzx_rng* r, const mzx_move* m, const int32_t* n_legal, const int32_t* words,
                        const int32_t* visit_counts, const double* temperature, const double* pow_table,
                        int32_t table_stride, const double* table_temperatures, int32_t num_temperatures,
                        int64_t* action) {
  int rc = move_check(r, m);
  if (rc) return rc;
  if (!n_legal || !visit_counts || !temperature || !action || num_temperatures < 0 ||
      (num_temperatures > 0 && (!pow_table || !table_temperatures || table_stride < 1))) {
    set_error("mzx_selfplay_select: missing argument");
    return MZX_ERR_INVALID;
  }
  const int B = m->num_games, A = m->action_space_size;
  if (A > 4096) { set_error("mzx_selfplay_select: more than 4096 actions"); return MZX_ERR_INVALID; }
  rc = select_check(m->legal_actions, n_legal, visit_counts, temperature, B, A, table_stride, table_temperatures, num_temperatures);
  if (rc) return rc;
  SelectArgs sa;
  sa.r = r; sa.idx = m->streams; sa.legal_all = m->legal_actions; sa.n_legal = n_legal; sa.words = words; sa.visit_counts = visit_counts;
  sa.temperature = temperature; sa.pow_table = pow_table; sa.table_stride = table_stride; sa.table_temperatures = table_temperatures;
  sa.num_temperatures = num_temperatures; sa.action = action; sa.A = A;
  rng_parallel(r, B, m->num_threads, [=](int lo, int hi) { select_range(sa, lo, hi); });
  return MZX_OK;
}

// ------------------------------------------------------------- self-play draws on the device (mzx_draws.h)

int mzx_selfplay_draws(const mzx_draws* d, void* stream) {
  const int rc = draws_check("mzx_selfplay_draws", d);
  if (rc) return rc;
  if (d->tape_words < 1) { set_error("mzx_selfplay_draws: tape_words %d must be at least 1", d->tape_words); return MZX_ERR_INVALID; }
  if (!d->d_tape) { set_error("mzx_selfplay_draws: d_tape missing"); return MZX_ERR_INVALID; }
  if (d->d_noise && !d->d_legal_actions && !d->d_n) {
    set_error("mzx_selfplay_draws: noise needs d_legal_actions or d_n");
    return MZX_ERR_INVALID;
  }
  if (d->d_noise && !(d->dirichlet_alpha > 0.0 && d->dirichlet_alpha <= 1.7976931348623157e308)) {
    set_error("mzx_selfplay_draws: dirichlet_alpha %g must be positive and finite", d->dirichlet_alpha);
    return MZX_ERR_INVALID;
  }
  SelfplayDrawsParams p;
  p.seed = d->seed; p.counter = d->counter; p.streams = d->d_streams; p.legal = d->d_legal_actions; p.n_rows = d->d_n;
  p.noise = d->d_noise; p.tape = d->d_tape; p.alpha = d->dirichlet_alpha; p.first_stream = d->first_stream;
  p.B = d->num_games; p.A = d->action_space_size; p.tape_words = d->tape_words;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(SelfplayDrawsBody{p}, (stream_t)stream));
  return MZX_OK;
}

int mzx_selfplay_select_device(const mzx_draws* d, const mzx_draws_select* sel, void* stream) {
  SelfplaySelectParams p;
  const int rc = draws_select_params("mzx_selfplay_select_device", d, sel, &p);
  if (rc) return rc;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(SelfplaySelectBody{p}, (stream_t)stream));
  return MZX_OK;
}

int mzx_selfplay_move_device(mzx_search* s, const mzx_move* m, const mzx_draws* d, const mzx_draws_select* sel, int32_t* n_legal,
                             void* d_arena, int64_t arena_bytes, void* stream) {
  const char* who = "mzx_selfplay_move_device";
  if (!m) { set_error("%s: null mzx_move", who); return MZX_ERR_INVALID; }
  if (!s) { set_error("%s: missing buffer", who); return MZX_ERR_INVALID; }
  SelfplaySelectParams sp;
  int rc = sel ? draws_select_params(who, d, sel, &sp, true) : draws_check(who, d);      // (no sel: no action choice)
  if (rc) return rc;
  if (m->num_games != d->num_games || m->action_space_size != d->action_space_size || m->tape_words != d->tape_words || m->tape_words < 1) {
    set_error("%s: the move and the draws disagree on num_games / action_space_size / tape_words (>= 1)", who);
    return MZX_ERR_INVALID;
  }
  const mzx_search_io& io = m->io;
  if (m->add_exploration_noise ? !io.d_noise : io.d_noise != nullptr) {
    set_error("%s: io.d_noise must be set with add_exploration_noise and NULL without", who);
    return MZX_ERR_INVALID;
  }
  if (!io.d_tape || !io.d_visit_counts) { set_error("%s: io.d_tape / io.d_visit_counts missing", who); return MZX_ERR_INVALID; }
  rc = move_stage(m, n_legal, who, false);
  if (rc == MZX_OK) rc = move_upload(m, stream);
  if (rc == MZX_OK) rc = actor_queue_device_move(s, m, d, sel, d_arena, arena_bytes, stream);
  return rc ? rc : move_finish(m, stream);
}

// ------------------------------------------------------------- replay hand-off: initial PER priorities on the device

int mzx_replay_priorities(const double* d_root_values, const double* d_rewards, const int32_t* d_to_play, int32_t num_games,
                          int32_t moves, int32_t td_steps, const double* d_discount_pow, double per_alpha, double* d_targets,
                          float* d_priorities, float* d_game_priority, void* stream) {
  if (num_games < 0 || moves < 0 || td_steps < 0) { set_error("mzx_replay_priorities: negative argument"); return MZX_ERR_INVALID; }
  if (num_games == 0 || moves == 0) return MZX_OK;
  if (!d_root_values || !d_rewards || !d_to_play || !d_discount_pow || !d_priorities) { set_error("mzx_replay_priorities: missing buffer"); return MZX_ERR_INVALID; }
  ReplayPriorityOp op;
  op.root_values = d_root_values; op.rewards = d_rewards; op.to_play = d_to_play; op.discount_pow = d_discount_pow;
  op.targets = d_targets; op.priorities = d_priorities; op.per_alpha = per_alpha;
  op.num_games = num_games; op.moves = moves; op.td_steps = td_steps;
  MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  if (d_game_priority) {
    ReplayGameMaxOp mx;
    mx.priorities = d_priorities; mx.game_priority = d_game_priority; mx.num_games = num_games; mx.moves = moves;
    MZX_TRY_LAUNCH(launch<64>(mx, (stream_t)stream));
  }
  return MZX_OK;
}

// ------------------------------------------------------------- device-resident replay store: values + batches

int mzx_replay_values(const mzx_replay_pool* pool, const int64_t* d_base, const int32_t* d_len, int32_t num_games,
                      int32_t td_steps, const double* d_discount_pow, void* stream) {
  if (!pool) { set_error("mzx_replay_values: null pool"); return MZX_ERR_INVALID; }
  if (num_games < 0 || td_steps < 0) { set_error("mzx_replay_values: negative argument"); return MZX_ERR_INVALID; }
  if (num_games == 0) return MZX_OK;
  if (!pool->d_root_values || !pool->d_rewards || !pool->d_to_play || !pool->d_values || !d_base || !d_len || !d_discount_pow) {
    set_error("mzx_replay_values: missing buffer");
    return MZX_ERR_INVALID;
  }
  ReplayValuesOp op;
  op.root_values = pool->d_root_values; op.rewards = pool->d_rewards; op.to_play = pool->d_to_play;
  op.discount_pow = d_discount_pow; op.values = pool->d_values; op.base = d_base; op.len = d_len;
  op.num_games = num_games; op.td_steps = td_steps;
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_positions(const int64_t* d_base, const int32_t* d_len, const int64_t* d_first, int32_t num_games,
                         int64_t total_positions, int64_t first, int32_t count, int64_t* d_sample_base, int32_t* d_sample_len,
                         int32_t* d_sample_pos, void* stream) {
  if (num_games < 0 || total_positions < 0 || first < 0 || count < 0) { set_error("mzx_replay_positions: negative argument"); return MZX_ERR_INVALID; }
  if (first + (int64_t)count > total_positions) {
    set_error("mzx_replay_positions: window [%lld, %lld) runs past the last of %lld positions", (long long)first,
              (long long)(first + count), (long long)total_positions);
    return MZX_ERR_INVALID;
  }
  if (count == 0) return MZX_OK;
  if (!d_base || !d_len || !d_first || !d_sample_base || !d_sample_len || !d_sample_pos) {
    set_error("mzx_replay_positions: missing buffer");
    return MZX_ERR_INVALID;
  }
  ReplayPositionsOp op;
  op.base = d_base; op.len = d_len; op.first = d_first; op.sample_base = d_sample_base; op.sample_len = d_sample_len;
  op.sample_pos = d_sample_pos; op.first_position = first; op.num_games = num_games; op.count = count;
  MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_reanalyse_write(const float* d_value_logits, int32_t num_samples, int32_t support_size, const int64_t* d_sample_base,
                               const int32_t* d_sample_pos, float* d_out, double* d_root_values, void* stream) {
  if (num_samples < 0 || support_size < 0) { set_error("mzx_replay_reanalyse_write: negative argument"); return MZX_ERR_INVALID; }
  if (num_samples == 0) return MZX_OK;
  if (!d_value_logits || !d_sample_base || !d_sample_pos || !d_out || !d_root_values) {
    set_error("mzx_replay_reanalyse_write: missing buffer");
    return MZX_ERR_INVALID;
  }
  ReplayReanalyseOp op;
  op.logits = d_value_logits; op.sample_base = d_sample_base; op.sample_pos = d_sample_pos; op.out = d_out;
  op.root_values = d_root_values; op.n = num_samples; op.support_size = support_size;
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_search_inputs(const mzx_replay_pool* pool, const uint32_t* d_legal_mask, const int64_t* d_sample_base,
                             const int32_t* d_sample_pos, int32_t num_samples, int32_t tape_words, uint64_t seed,
                             uint64_t sweep_counter, int64_t first_index, int32_t* d_to_play, int32_t* d_legal, uint32_t* d_tape,
                             int32_t* d_input_flags, void* stream) {
  if (!pool) { set_error("mzx_replay_search_inputs: null pool"); return MZX_ERR_INVALID; }
  if (num_samples < 0 || tape_words < 1 || pool->action_space_size < 1 || pool->rows < 1) {
    set_error("mzx_replay_search_inputs: num_samples %d must not be negative, tape_words %d, action_space_size %d and rows %lld positive",
              num_samples, tape_words, pool->action_space_size, (long long)pool->rows);
    return MZX_ERR_INVALID;
  }
  if (first_index < 0 || first_index + (int64_t)num_samples > ((int64_t)1 << 32)) {
    set_error("mzx_replay_search_inputs: positions [%lld, %lld) leave the 32-bit index of the tape's counter", (long long)first_index,
              (long long)(first_index + num_samples));
    return MZX_ERR_INVALID;
  }
  if (!pool->d_to_play || !d_sample_base || !d_sample_pos || !d_to_play || !d_legal || !d_tape || !d_input_flags) {
    set_error("mzx_replay_search_inputs: missing buffer");
    return MZX_ERR_INVALID;
  }
  if (num_samples == 0) return MZX_OK;
  ReplaySearchInputsBody b;
  b.pool_to_play = pool->d_to_play; b.legal_mask = d_legal_mask; b.sample_base = d_sample_base; b.sample_pos = d_sample_pos;
  b.to_play = d_to_play; b.legal = d_legal; b.tape = d_tape; b.flags = d_input_flags; b.seed = seed; b.sweep_counter = sweep_counter;
  b.first_index = first_index; b.rows = pool->rows; b.n = num_samples; b.A = pool->action_space_size; b.tape_words = tape_words;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(b, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_search_write(const int32_t* d_visit_counts, const double* d_root_value, const int32_t* d_info,
                            const int32_t* d_input_flags, int32_t num_samples, int32_t action_space_size,
                            const int64_t* d_sample_base, const int32_t* d_sample_pos, double* d_child_visits,
                            double* d_root_values, int32_t* d_skipped, void* stream) {
  if (num_samples < 0 || action_space_size < 1) {
    set_error("mzx_replay_search_write: num_samples %d must not be negative, action_space_size %d positive", num_samples, action_space_size);
    return MZX_ERR_INVALID;
  }
  if (!d_visit_counts || !d_root_value || !d_info || !d_input_flags || !d_sample_base || !d_sample_pos || !d_child_visits ||
      !d_root_values || !d_skipped) {
    set_error("mzx_replay_search_write: missing buffer");
    return MZX_ERR_INVALID;
  }
  if (num_samples == 0) return MZX_OK;
  ReplaySearchWriteBody b;
  b.visits = d_visit_counts; b.root_value = d_root_value; b.info = d_info; b.flags = d_input_flags; b.sample_base = d_sample_base;
  b.sample_pos = d_sample_pos; b.child_visits = d_child_visits; b.root_values = d_root_values; b.skipped = d_skipped;
  b.n = num_samples; b.A = action_space_size;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(b, (stream_t)stream));
  return MZX_OK;
}

extern "C++" {
template <int VEC>
static int replay_obs_launch(const mzx_replay_pool* pool, const mzx_replay_batch_io* io, stream_t stream) {
  ReplayObsOp<VEC> op;
  op.frames = pool->d_frames; op.actions = pool->d_actions; op.base = io->d_base; op.pos = io->d_pos; op.out = io->d_observation;
  op.C = pool->channels; op.hwv = pool->height * pool->width / VEC; op.k = io->stacked_observations;
  op.A = pool->action_space_size; op.n_out = io->num_samples;
  op.c_out = pool->channels * (io->stacked_observations + 1) + io->stacked_observations;
  op.pieces = (op.hwv + 64 * OBS_UNROLL - 1) / (64 * OBS_UNROLL);
  if ((int64_t)op.n_out * op.c_out * op.pieces >= (int64_t)1 << 26) {   // 32-bit group index; split the call
    set_error("mzx_replay_batch: %d samples x %d planes exceed one launch; gather in smaller batches", op.n_out, op.c_out);
    return MZX_ERR_INVALID;
  }
  MZX_TRY_LAUNCH(launch<256>(op, stream));
  return MZX_OK;
}
}  // extern "C++"

int mzx_replay_batch(const mzx_replay_pool* pool, const mzx_replay_batch_io* io, void* stream) {
  if (!pool || !io) { set_error("mzx_replay_batch: null argument"); return MZX_ERR_INVALID; }
  if (io->num_samples < 0 || io->num_unroll_steps < 0 || io->stacked_observations < 0) {
    set_error("mzx_replay_batch: negative argument");
    return MZX_ERR_INVALID;
  }
  if (pool->action_space_size <= 0) { set_error("mzx_replay_batch: action_space_size must be positive"); return MZX_ERR_INVALID; }
  if (io->num_samples == 0) return MZX_OK;
  if (!io->d_base || !io->d_len || !io->d_pos) { set_error("mzx_replay_batch: missing sample arrays"); return MZX_ERR_INVALID; }
  if (io->d_observation) {
    if (pool->channels < 1 || pool->height < 1 || pool->width < 1 ||
        (int64_t)pool->channels * (io->stacked_observations + 1) + io->stacked_observations >= (1 << 20)) {
      set_error("mzx_replay_batch: invalid observation shape %d x %d x %d", pool->channels, pool->height, pool->width);
      return MZX_ERR_INVALID;
    }
    if (!pool->d_frames || (io->stacked_observations > 0 && !pool->d_actions)) { set_error("mzx_replay_batch: missing pool frames / actions"); return MZX_ERR_INVALID; }
    const bool vec = (pool->height * pool->width) % 4 == 0 && ((uintptr_t)pool->d_frames % 16) == 0 &&
                     ((uintptr_t)io->d_observation % 16) == 0;
    const int rc = vec ? replay_obs_launch<4>(pool, io, (stream_t)stream) : replay_obs_launch<1>(pool, io, (stream_t)stream);
    if (rc) return rc;
  }
  if (io->d_value) {
    if (!io->d_reward || !io->d_policy || !io->d_action || !io->d_gradient_scale || !io->d_absorbing_actions || !pool->d_actions ||
        !pool->d_rewards || !pool->d_child_visits || !pool->d_values) {
      set_error("mzx_replay_batch: missing target buffer");
      return MZX_ERR_INVALID;
    }
    ReplayTargetsOp op;
    op.actions = pool->d_actions; op.rewards = pool->d_rewards; op.child_visits = pool->d_child_visits; op.values = pool->d_values;
    op.base = io->d_base; op.len = io->d_len; op.pos = io->d_pos; op.absorbing = io->d_absorbing_actions;
    op.value = io->d_value; op.reward = io->d_reward; op.policy = io->d_policy; op.action = io->d_action;
    op.gradient_scale = io->d_gradient_scale; op.n = io->num_samples; op.U = io->num_unroll_steps; op.A = pool->action_space_size;
    MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  }
  return MZX_OK;
}

// ------------------------------------------------------------- device replay store: prioritised draws + priority feedback

static int replay_sampler_table(const char* who, const mzx_replay_sampler* sampler, ReplaySamplerTable* t) {
  if (!sampler) { set_error("%s: null sampler", who); return MZX_ERR_INVALID; }
  if (sampler->rows < 1 || sampler->slots < 1) { set_error("%s: rows and slots must be positive", who); return MZX_ERR_INVALID; }
  if (!sampler->d_priorities || !sampler->d_owner || !sampler->d_slot_game || !sampler->d_slot_base || !sampler->d_slot_len ||
      !sampler->d_slot_priority || !sampler->d_slot_sum) {
    set_error("%s: missing sampler column", who);
    return MZX_ERR_INVALID;
  }
  t->priorities = sampler->d_priorities; t->owner = sampler->d_owner; t->slot_game = sampler->d_slot_game;
  t->slot_base = sampler->d_slot_base; t->slot_len = sampler->d_slot_len; t->slot_priority = sampler->d_slot_priority;
  t->slot_sum = sampler->d_slot_sum; t->rows = sampler->rows; t->slots = sampler->slots;
  return MZX_OK;
}

int mzx_replay_sampler_refresh(const mzx_replay_sampler* sampler, const int32_t* d_slots, int32_t n, void* stream) {
  ReplayRefreshParams p;
  const int rc = replay_sampler_table("mzx_replay_sampler_refresh", sampler, &p.t);
  if (rc) return rc;
  if (n < 0) { set_error("mzx_replay_sampler_refresh: negative count"); return MZX_ERR_INVALID; }
  if (n == 0) return MZX_OK;
  if (!d_slots) { set_error("mzx_replay_sampler_refresh: missing slot list"); return MZX_ERR_INVALID; }
  p.slot_list = d_slots; p.game_ids = nullptr; p.n = n;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayRefreshBody{p}, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_sample(const mzx_replay_sampler* sampler, const mzx_replay_sample_io* io, void* stream) {
  ReplayDrawParams p;
  const int rc = replay_sampler_table("mzx_replay_sample", sampler, &p.t);
  if (rc) return rc;
  if (!io) { set_error("mzx_replay_sample: null io"); return MZX_ERR_INVALID; }
  if (io->num_samples < 0 || io->num_unroll_steps < 0 || io->num_actions < 1) {
    set_error("mzx_replay_sample: num_samples %d and num_unroll_steps %d must not be negative, num_actions %d positive",
              io->num_samples, io->num_unroll_steps, io->num_actions);
    return MZX_ERR_INVALID;
  }
  if (!io->d_base || !io->d_len || !io->d_pos || !io->d_absorbing_actions || !io->d_game_id || (io->per && !io->d_weight)) {
    set_error("mzx_replay_sample: missing output");
    return MZX_ERR_INVALID;
  }
  if (!sampler->d_tile_prefix || (io->per && (!sampler->d_raw || sampler->raw_capacity < io->num_samples))) {
    set_error("mzx_replay_sample: workspace missing or short (%lld raw entries for %d samples)", (long long)sampler->raw_capacity,
              io->num_samples);
    return MZX_ERR_INVALID;
  }
  if (io->num_samples == 0) return MZX_OK;
  p.tile_prefix = sampler->d_tile_prefix; p.raw = sampler->d_raw; p.action_space = io->d_action_space; p.uniforms = io->d_uniforms;
  p.out_base = io->d_base; p.out_len = io->d_len; p.out_pos = io->d_pos; p.out_tape = io->d_absorbing_actions;
  p.out_game = io->d_game_id; p.out_weight = io->d_weight; p.seed = io->seed; p.call_counter = io->call_counter;
  p.total_samples = io->total_samples; p.n = io->num_samples; p.per = io->per ? 1 : 0; p.U = io->num_unroll_steps;
  p.A = io->num_actions; p.tiles = (sampler->slots + SAMPLER_TILE - 1) / SAMPLER_TILE;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayTileSumBody{p}, (stream_t)stream));
  MZX_TRY_LAUNCH(launch_waves<2>(ReplayTilePrefixBody{p}, (stream_t)stream));
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayDrawBody{p}, (stream_t)stream));
  if (p.per) MZX_TRY_LAUNCH(launch_block<SAMPLER_FINISH_BLOCK>(ReplayWeightFinishBody{p}, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_update_priorities(const mzx_replay_sampler* sampler, const float* d_new, const int64_t* d_game_id,
                                 const int32_t* d_pos, int32_t n, int32_t steps, void* stream) {
  ReplayClaimOp op;
  const int rc = replay_sampler_table("mzx_replay_update_priorities", sampler, &op.t);
  if (rc) return rc;
  if (n < 0 || steps < 1) { set_error("mzx_replay_update_priorities: n %d must not be negative, steps %d positive", n, steps); return MZX_ERR_INVALID; }
  if (n == 0) return MZX_OK;
  if (!d_new || !d_game_id || !d_pos) { set_error("mzx_replay_update_priorities: missing buffer"); return MZX_ERR_INVALID; }
  op.fresh = d_new; op.game_id = d_game_id; op.pos = d_pos; op.n = n; op.steps = steps;
  op.write = 0;
  MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  op.write = 1;
  MZX_TRY_LAUNCH(launch<256>(op, (stream_t)stream));
  ReplayRefreshParams p;
  p.t = op.t; p.slot_list = nullptr; p.game_ids = d_game_id; p.n = n;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayRefreshBody{p}, (stream_t)stream));
  return MZX_OK;
}

int mzx_replay_ingest(const mzx_replay_pool* pool, const mzx_replay_sampler* sampler, uint32_t* d_pool_legal_mask,
                      int64_t mask_rows, const mzx_replay_ingest_io* io, void* stream) {
  if (!pool || !io) { set_error("mzx_replay_ingest: null argument"); return MZX_ERR_INVALID; }
  if (io->num_games < 0 || io->td_steps < 0 || io->total_rows < io->num_games) {
    set_error("mzx_replay_ingest: num_games %d and td_steps %d must not be negative, total_rows %lld at least num_games",
              io->num_games, io->td_steps, (long long)io->total_rows);
    return MZX_ERR_INVALID;
  }
  if (pool->rows < 1 || pool->action_space_size < 1 || pool->channels < 1 || pool->height < 1 || pool->width < 1) {
    set_error("mzx_replay_ingest: the pool's rows, action space and observation shape must be positive");
    return MZX_ERR_INVALID;
  }
  if (io->action_space_size != pool->action_space_size || io->channels != pool->channels || io->height != pool->height ||
      io->width != pool->width) {
    set_error("mzx_replay_ingest: staged games of %d actions and %d x %d x %d frames, the pool holds %d and %d x %d x %d",
              io->action_space_size, io->channels, io->height, io->width, pool->action_space_size, pool->channels, pool->height,
              pool->width);
    return MZX_ERR_INVALID;
  }
  const int64_t frame_floats = (int64_t)pool->channels * pool->height * pool->width;
  if (frame_floats >= ((int64_t)1 << 31)) { set_error("mzx_replay_ingest: frame too large"); return MZX_ERR_INVALID; }
  if (d_pool_legal_mask && mask_rows != pool->rows) {
    set_error("mzx_replay_ingest: the mask column has %lld rows, the pool %lld", (long long)mask_rows, (long long)pool->rows);
    return MZX_ERR_INVALID;
  }
  ReplayIngestSlotBody slots;
  if (sampler) {
    const int rc = replay_sampler_table("mzx_replay_ingest", sampler, &slots.t);
    if (rc) return rc;
    if (sampler->rows != pool->rows) {
      set_error("mzx_replay_ingest: the sampler has %lld rows, the pool %lld", (long long)sampler->rows, (long long)pool->rows);
      return MZX_ERR_INVALID;
    }
  }
  if (io->num_games == 0) return MZX_OK;
  if (!pool->d_frames || !pool->d_actions || !pool->d_rewards || !pool->d_to_play || !pool->d_root_values ||
      !pool->d_child_visits || !pool->d_values) {
    set_error("mzx_replay_ingest: missing pool column");
    return MZX_ERR_INVALID;
  }
  if (!io->d_len || !io->d_base || !io->d_game_id || !io->d_src1 || !io->d_src0 || !io->d_observations || !io->d_actions ||
      !io->d_rewards || !io->d_to_play || !io->d_visits || !io->d_root_values || !io->d_discount_pow) {
    set_error("mzx_replay_ingest: missing staged array");
    return MZX_ERR_INVALID;
  }
  const bool per = sampler && io->per;
  ReplayIngestParams p;
  p.len = io->d_len; p.base = io->d_base; p.game_id = io->d_game_id; p.src1 = io->d_src1; p.src0 = io->d_src0;
  p.observations = io->d_observations; p.actions = io->d_actions; p.rewards = io->d_rewards; p.to_play = io->d_to_play;
  p.visits = io->d_visits; p.root_values = io->d_root_values; p.legal = io->d_legal_mask;
  p.staged_priorities = per ? io->d_priorities : nullptr;
  // the pool's columns, writable here (the struct holds them const for the entries that read them)
  p.pool_frames = const_cast<float*>(pool->d_frames); p.pool_actions = const_cast<int32_t*>(pool->d_actions);
  p.pool_rewards = const_cast<double*>(pool->d_rewards); p.pool_to_play = const_cast<int32_t*>(pool->d_to_play);
  p.pool_root_values = const_cast<double*>(pool->d_root_values); p.pool_child_visits = const_cast<double*>(pool->d_child_visits);
  p.pool_mask = d_pool_legal_mask; p.pool_priorities = sampler ? sampler->d_priorities : nullptr;
  p.rows = pool->rows; p.total_rows = io->total_rows; p.G = io->num_games; p.A = pool->action_space_size;
  p.frame_floats = (int32_t)frame_floats; p.per = per ? 1 : 0;
  p.vec = frame_floats % 4 == 0 && ((uintptr_t)io->d_observations % 16) == 0 && ((uintptr_t)pool->d_frames % 16) == 0;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayIngestRowBody{p}, (stream_t)stream));
  ReplayValuesOp op;
  op.root_values = pool->d_root_values; op.rewards = pool->d_rewards; op.to_play = pool->d_to_play;
  op.discount_pow = io->d_discount_pow; op.values = pool->d_values; op.base = io->d_base; op.len = io->d_len;
  op.num_games = io->num_games; op.td_steps = io->td_steps; op.rows = pool->rows;
  if (per && !io->d_priorities) { op.priorities = sampler->d_priorities; op.per_alpha = io->per_alpha; }
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  if (sampler) {
    slots.slot_game = const_cast<int64_t*>(sampler->d_slot_game); slots.slot_base = const_cast<int64_t*>(sampler->d_slot_base);
    slots.slot_len = const_cast<int32_t*>(sampler->d_slot_len);
    slots.game_id = io->d_game_id; slots.base = io->d_base; slots.len = io->d_len; slots.n = io->num_games;
    MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(slots, (stream_t)stream));
  }
  return MZX_OK;
}

int mzx_replay_export(const mzx_replay_pool* pool, const mzx_replay_sampler* sampler, const uint32_t* d_pool_legal_mask,
                      int64_t mask_rows, const mzx_replay_export_io* io, void* stream) {
  if (!pool || !io) { set_error("mzx_replay_export: null argument"); return MZX_ERR_INVALID; }
  if (io->num_games < 0 || io->total_rows < io->num_games) {
    set_error("mzx_replay_export: num_games %d must not be negative, total_rows %lld at least num_games", io->num_games,
              (long long)io->total_rows);
    return MZX_ERR_INVALID;
  }
  if (pool->rows < 1 || pool->action_space_size < 1 || pool->channels < 1 || pool->height < 1 || pool->width < 1) {
    set_error("mzx_replay_export: the pool's rows, action space and observation shape must be positive");
    return MZX_ERR_INVALID;
  }
  const int64_t frame_floats = (int64_t)pool->channels * pool->height * pool->width;
  if (frame_floats >= ((int64_t)1 << 31)) { set_error("mzx_replay_export: frame too large"); return MZX_ERR_INVALID; }
  if (io->d_legal_mask && (!d_pool_legal_mask || mask_rows != pool->rows)) {
    set_error("mzx_replay_export: the legal mask needs the pool's mask column: it has %lld rows, the pool %lld",
              (long long)(d_pool_legal_mask ? mask_rows : 0), (long long)pool->rows);
    return MZX_ERR_INVALID;
  }
  if (io->d_priorities && (!sampler || !sampler->d_priorities || sampler->rows != pool->rows)) {
    set_error("mzx_replay_export: the priorities need the sampler's column: it has %lld rows, the pool %lld",
              (long long)(sampler && sampler->d_priorities ? sampler->rows : 0), (long long)pool->rows);
    return MZX_ERR_INVALID;
  }
  if (io->num_games == 0) return MZX_OK;
  if (!pool->d_frames || !pool->d_actions || !pool->d_rewards || !pool->d_to_play || !pool->d_root_values || !pool->d_child_visits) {
    set_error("mzx_replay_export: missing pool column");
    return MZX_ERR_INVALID;
  }
  if (!io->d_base || !io->d_len || !io->d_dst1 || !io->d_dst0 || !io->d_observations || !io->d_actions || !io->d_rewards ||
      !io->d_to_play || !io->d_child_visits || !io->d_root_values) {
    set_error("mzx_replay_export: missing packed array");
    return MZX_ERR_INVALID;
  }
  ReplayExportParams p;
  p.base = io->d_base; p.len = io->d_len; p.dst1 = io->d_dst1; p.dst0 = io->d_dst0;
  p.pool_frames = pool->d_frames; p.pool_actions = pool->d_actions; p.pool_rewards = pool->d_rewards;
  p.pool_to_play = pool->d_to_play; p.pool_root_values = pool->d_root_values; p.pool_child_visits = pool->d_child_visits;
  p.pool_mask = io->d_legal_mask ? d_pool_legal_mask : nullptr;
  p.pool_priorities = io->d_priorities ? sampler->d_priorities : nullptr;
  p.observations = io->d_observations; p.actions = io->d_actions; p.rewards = io->d_rewards; p.to_play = io->d_to_play;
  p.child_visits = io->d_child_visits; p.root_values = io->d_root_values; p.legal = io->d_legal_mask;
  p.priorities = io->d_priorities;
  p.rows = pool->rows; p.total_rows = io->total_rows; p.G = io->num_games; p.A = pool->action_space_size;
  p.frame_floats = (int32_t)frame_floats;
  p.vec = frame_floats % 4 == 0 && ((uintptr_t)io->d_observations % 16) == 0 && ((uintptr_t)pool->d_frames % 16) == 0;
  MZX_TRY_LAUNCH(launch_waves<SAMPLER_WAVES>(ReplayExportRowBody{p}, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------------- the trainer's loss head (csrc/mzx_trainer.h)

int mzx_scalar_to_support(const float* d_x, int32_t rows, int32_t support_size, float* d_out, void* stream) {
  if (rows < 0 || support_size < 0) { set_error("scalar_to_support: negative argument"); return MZX_ERR_INVALID; }
  if (rows == 0) return MZX_OK;
  if (!d_x || !d_out) { set_error("scalar_to_support: missing buffer"); return MZX_ERR_INVALID; }
  ScalarToSupportOp op;
  op.x = d_x; op.out = d_out; op.rows = rows; op.support_size = support_size;
  MZX_TRY_LAUNCH(launch<64>(op, (stream_t)stream));
  return MZX_OK;
}

int64_t mzx_trainer_loss_scratch_bytes(int32_t batch, int32_t steps) {
  if (batch < 1 || steps < 1) return 0;
  return (int64_t)sizeof(TrainerLossRow) * batch * steps;
}

int mzx_trainer_loss(const mzx_trainer_loss_io* io, void* stream) {
  if (!io) { set_error("mzx_trainer_loss: null argument"); return MZX_ERR_INVALID; }
  if (io->batch < 1 || io->steps < 1 || io->num_actions < 1 || io->support_size < 0) {
    set_error("mzx_trainer_loss: batch %d, steps %d, num_actions %d must be positive, support_size %d not negative", io->batch,
              io->steps, io->num_actions, io->support_size);
    return MZX_ERR_INVALID;
  }
  if (!io->d_value_logits || !io->d_reward_logits || !io->d_policy_logits || !io->d_target_value || !io->d_target_reward ||
      !io->d_target_policy || !io->d_gradient_scale || !io->d_losses || !io->d_priorities || !io->d_scratch) {
    set_error("mzx_trainer_loss: missing buffer");
    return MZX_ERR_INVALID;
  }
  const int given = (io->d_grad_value != nullptr) + (io->d_grad_reward != nullptr) + (io->d_grad_policy != nullptr);
  if (given != 0 && given != 3) { set_error("mzx_trainer_loss: the three gradient buffers go together"); return MZX_ERR_INVALID; }
  const int64_t rows = (int64_t)io->batch * io->steps;
  if (io->scratch_bytes < mzx_trainer_loss_scratch_bytes(io->batch, io->steps) || ((uintptr_t)io->d_scratch % 16) != 0) {
    set_error("mzx_trainer_loss: scratch needs %lld bytes, 16-byte aligned", (long long)mzx_trainer_loss_scratch_bytes(io->batch, io->steps));
    return MZX_ERR_INVALID;
  }
  if (rows >= ((int64_t)1 << 31)) { set_error("mzx_trainer_loss: batch x steps exceeds one launch"); return MZX_ERR_INVALID; }
  TrainerLossParams p;
  p.value_logits = io->d_value_logits; p.reward_logits = io->d_reward_logits; p.policy_logits = io->d_policy_logits;
  p.target_value = io->d_target_value; p.target_reward = io->d_target_reward; p.target_policy = io->d_target_policy;
  p.gradient_scale = io->d_gradient_scale; p.weight = io->d_weight; p.priorities = io->d_priorities;
  p.grad_value = io->d_grad_value; p.grad_reward = io->d_grad_reward; p.grad_policy = io->d_grad_policy;
  p.scratch = (TrainerLossRow*)io->d_scratch; p.losses = io->d_losses;
  p.batch = io->batch; p.steps = io->steps; p.support_size = io->support_size; p.num_actions = io->num_actions;
  p.value_loss_weight = (float)io->value_loss_weight; p.per_alpha = (float)io->per_alpha;
  MZX_TRY_LAUNCH(launch_waves<TRAINER_WAVES>(TrainerLossBody{p}, (stream_t)stream));
  MZX_TRY_LAUNCH(launch_block<TRAINER_FINISH_BLOCK>(TrainerFinishBody{p}, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------------- a training step of a fully connected network (csrc/mzx_train_fc.h)
// Both step entries refuse through train_step_front and call the loss head through train_head_io (csrc/mzx_train_step.h).

int mzx_train_fc_supported(const mzx_net* net, int32_t batch, int32_t steps) {
  return (int)train_full_plan<FctPlan>(fct_plan, net, batch, steps, [](const FctPlan&) { return 1; });
}

int64_t mzx_train_fc_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps) {
  return train_full_plan<FctPlan>(fct_plan, net, batch, steps, [](const FctPlan& P) { return P.total_floats * 4; });
}

int mzx_train_fc_step(const mzx_net* net, const mzx_train_fc_io* io, void* stream) {
  FctParams p;
  if (const int rc = train_step_front("mzx_train_fc_step", net, io, false, fct_plan, p.plan)) return rc;
  float* scratch = (float*)io->d_scratch;
  const mzx_trainer_loss_io lio = train_head_io(io, p.plan, scratch, net->cfg.support_size, p.vlog, p.rlog, p.plog);
  p.flat = io->d_flat; p.obs = io->d_observation; p.action = io->d_action;
  p.gv = lio.d_grad_value; p.gr = lio.d_grad_reward; p.gp = lio.d_grad_policy;
  p.scratch = scratch; p.grad_flat = io->d_grad_flat;
  p.B = io->batch; p.steps = io->steps;
  MZX_TRY_LAUNCH(fct_launch(p, 0, (stream_t)stream));
  if (const int rc = mzx_trainer_loss(&lio, stream)) return rc;
  MZX_TRY_LAUNCH(fct_launch(p, 1, (stream_t)stream));
  MZX_TRY_LAUNCH(launch_waves<FCT_WAVES>(FctWgradBody{p}, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------------- a training step of a residual network (csrc/mzx_train_resnet.h)

int mzx_train_resnet_supported(const mzx_net* net, int32_t batch, int32_t steps) {
  return (int)train_full_plan<RtnPlan>(rtn_plan, net, batch, steps, [](const RtnPlan&) { return 1; });
}

int64_t mzx_train_resnet_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps) {
  return train_full_plan<RtnPlan>(rtn_plan, net, batch, steps, [](const RtnPlan& P) { return P.total_floats * 4; });
}

int64_t mzx_train_resnet_stat_floats(const mzx_net* net) { return net ? rtn_stat_floats(net) : 0; }

int64_t mzx_train_resnet_launches(const mzx_net* net, int32_t batch, int32_t steps) {
  return train_full_plan<RtnPlan>(rtn_plan, net, batch, steps, [](const RtnPlan& plan) {
    RtnRun<false> run;      // (the launches of a step do not depend on its precision)
    memset((void*)&run, 0, sizeof(run));
    run.P = &plan; run.dry = true;
    run.forward();
    run.backward();
    return run.launched + 2;      // (the two launches of the loss head)
  });
}

// forward pass, loss head, backward pass of a planned step
extern "C++" template <bool WIDE>
int rtn_step(const mzx_net* net, const mzx_train_resnet_io* io, const RtnPlan& P, void* stream) {
  float* scratch = (float*)io->d_scratch;
  RtnRun<WIDE> run;
  memset((void*)&run, 0, sizeof(run));
  run.P = &P; run.flat = io->d_flat; run.obs = io->d_observation; run.action = io->d_action;
  run.scratch = scratch; run.grad = io->d_grad_flat; run.stats = io->d_stats; run.stream = (stream_t)stream;
  const mzx_trainer_loss_io lio = train_head_io(reinterpret_cast<const mzx_train_fc_io*>(io), P, scratch, net->cfg.support_size,
                                                run.vlog, run.rlog, run.plog);
  run.forward();
  MZX_TRY_LAUNCH(run.rc);
  if (const int rc = mzx_trainer_loss(&lio, stream)) return rc;
  run.backward();
  MZX_TRY_LAUNCH(run.rc);
  return MZX_OK;
}

int mzx_train_resnet_step(const mzx_net* net, const mzx_train_resnet_io* io, void* stream) {
  RtnPlan P;
  if (const int rc = train_step_front("mzx_train_resnet_step", net, reinterpret_cast<const mzx_train_fc_io*>(io), true, rtn_plan, P))
    return rc;
  return P.stem ? rtn_step<true>(net, io, P, stream) : rtn_step<false>(net, io, P, stream);
}

int mzx_net_set_train_stem(mzx_net* net, int on) {
  if (!net) { set_error("mzx_net_set_train_stem: null network handle"); return MZX_ERR_INVALID; }
  if (net->cfg.network != 1) { set_error("mzx_net_set_train_stem: fully connected networks have no downsample stem"); return MZX_ERR_INVALID; }
  net->train_stem = on ? 1 : 0;
  return MZX_OK;
}

int mzx_net_train_stem(const mzx_net* net) { return net ? net->train_stem : 0; }

int mzx_train_resnet_commit_stats(const mzx_net* net, const float* d_stats, float* d_flat_out, void* stream) {
  if (!net || !d_stats || !d_flat_out) { set_error("mzx_train_resnet_commit_stats: null argument"); return MZX_ERR_INVALID; }
  int64_t at = 0;
  for (const BnRef& b : net->bns) {
    if (b.var != b.mean + b.channels) { set_error("mzx_train_resnet_commit_stats: unexpected weight table"); return MZX_ERR_INVALID; }
    MZX_TRY_LAUNCH(copy_d2d(d_flat_out + b.mean, d_stats + at, sizeof(float) * 2 * b.channels, (stream_t)stream));
    at += 2 * (int64_t)b.channels;
  }
  return MZX_OK;
}

// ------------------------------------------------------------- the optimizer step over the flat buffer (csrc/mzx_optim.h)

int64_t mzx_optim_chunks(const int64_t* h_spans, int32_t num_spans, int64_t n, int64_t* h_chunks, int64_t cap) {
  if (!optim_spans_ok("mzx_optim_chunks", h_spans, num_spans, n)) return MZX_ERR_INVALID;
  int64_t at = 0;
  return optim_cut_chunks(h_spans, num_spans, [&](int64_t off, int64_t count) {
    if (h_chunks && at < cap) { h_chunks[2 * at] = off; h_chunks[2 * at + 1] = count; }
    ++at;
  });
}

int mzx_optim_step(const mzx_optim_io* io, void* stream) {
  if (const int rc = optim_check(io)) return rc;
  MZX_TRY_LAUNCH(optim_launch(io, (stream_t)stream));
  return MZX_OK;
}

// ------------------------------------------------------------- whole training steps behind one call (csrc/mzx_train_chain.h)

static int64_t chain_step_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps) {
  if (!net) return 0;
  return net->cfg.network == 1 ? mzx_train_resnet_scratch_bytes(net, batch, steps) : mzx_train_fc_scratch_bytes(net, batch, steps);
}

int mzx_train_chain_supported(const mzx_net* net, int32_t batch, int32_t steps) {
  if (!net) return 0;
  return net->cfg.network == 1 ? mzx_train_resnet_supported(net, batch, steps) : mzx_train_fc_supported(net, batch, steps);
}

int64_t mzx_train_chain_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps) {
  const int64_t step_bytes = chain_step_scratch_bytes(net, batch, steps);
  if (step_bytes <= 0) return 0;
  return chain_plan(net, batch, steps, step_bytes, net->cfg.network == 1 ? rtn_stat_floats(net) : 0).total_bytes;
}

int mzx_train_chain(mzx_net* net, const mzx_train_chain_io* io, void* stream) {
  const char* who = "mzx_train_chain";
  if (!net || !io) { set_error("%s: null argument", who); return MZX_ERR_INVALID; }
  if (io->num_steps < 1 || io->batch < 1 || io->num_unroll_steps < 0) {
    set_error("%s: num_steps %d and batch %d must be positive, num_unroll_steps %d not negative", who, io->num_steps, io->batch, io->num_unroll_steps);
    return MZX_ERR_INVALID;
  }
  if (!io->pool || !io->sampler || !io->d_flat || !io->d_grad_flat || !io->d_losses || !io->d_derived || !io->d_workspace) {
    set_error("%s: missing buffer", who);
    return MZX_ERR_INVALID;
  }
  const bool residual = net->cfg.network == 1, adam = io->optim.kind == MZX_OPTIM_ADAM;
  const int32_t B = io->batch, steps = io->num_unroll_steps + 1;
  if (!mzx_train_chain_supported(net, B, steps)) {
    set_error("%s: mzx_train_%s_step does not run this network at batch %d x %d steps", who, residual ? "resnet" : "fc", B, steps);
    return MZX_ERR_INVALID;
  }
  const mzx_replay_pool& pool = *io->pool;
  const int64_t planes = (int64_t)pool.channels * (io->stacked_observations + 1) + io->stacked_observations;
  if (io->stacked_observations < 0 || planes * pool.height * pool.width != net->input_size || pool.action_space_size != net->cfg.action_space_size ||
      io->num_actions != pool.action_space_size) {
    set_error("%s: the pool's stacked observation / action space is not the network's", who);
    return MZX_ERR_INVALID;
  }
  ReplaySamplerTable table;
  if (const int rc = replay_sampler_table(who, io->sampler, &table)) return rc;
  if (!io->sampler->d_tile_prefix || (io->per && (!io->sampler->d_raw || io->sampler->raw_capacity < B))) {
    set_error("%s: sampler workspace missing or short", who);
    return MZX_ERR_INVALID;
  }
  const ChainPlan P = chain_plan(net, B, steps, chain_step_scratch_bytes(net, B, steps), residual ? rtn_stat_floats(net) : 0);
  if (io->workspace_bytes < P.total_bytes || ((uintptr_t)io->d_workspace % 256) != 0) {
    set_error("%s: workspace needs %lld bytes, 256-byte aligned", who, (long long)P.total_bytes);
    return MZX_ERR_INVALID;
  }
  if (io->derived_floats < derived_total(net)) { set_error("%s: derived buffer too small", who); return MZX_ERR_INVALID; }
  if (io->optim.d_param != io->d_flat || io->optim.d_grad != io->d_grad_flat || io->optim.n != net->num_params) {
    set_error("%s: the optimizer must step d_flat with d_grad_flat (%lld elements)", who, (long long)net->num_params);
    return MZX_ERR_INVALID;
  }
  if (adam ? (!io->h_step_size || !io->h_bias_correction2_sqrt) : !io->h_lr) { set_error("%s: missing per-step scalars", who); return MZX_ERR_INVALID; }
  if (const int rc = optim_check(&io->optim)) return rc;      // (t only grows: the later steps pass what step 0 passes)

  char* ws = (char*)io->d_workspace;
  mzx_replay_sample_io sio;
  memset(&sio, 0, sizeof(sio));
  sio.seed = io->seed; sio.total_samples = io->total_samples; sio.num_samples = B; sio.per = io->per ? 1 : 0;
  sio.num_unroll_steps = io->num_unroll_steps; sio.num_actions = io->num_actions; sio.d_action_space = io->d_action_space;
  sio.d_base = (int64_t*)(ws + P.base); sio.d_len = (int32_t*)(ws + P.len); sio.d_pos = (int32_t*)(ws + P.pos);
  sio.d_absorbing_actions = (int32_t*)(ws + P.tape); sio.d_game_id = (int64_t*)(ws + P.game_id);
  sio.d_weight = io->per ? (float*)(ws + P.weight) : nullptr;
  mzx_replay_batch_io bio;
  memset(&bio, 0, sizeof(bio));
  bio.d_base = sio.d_base; bio.d_len = sio.d_len; bio.d_pos = sio.d_pos; bio.d_absorbing_actions = sio.d_absorbing_actions;
  bio.num_samples = B; bio.num_unroll_steps = io->num_unroll_steps; bio.stacked_observations = io->stacked_observations;
  bio.d_observation = (float*)(ws + P.obs); bio.d_value = (double*)(ws + P.value64); bio.d_reward = (double*)(ws + P.reward64);
  bio.d_policy = (double*)(ws + P.policy64); bio.d_action = (int64_t*)(ws + P.action64); bio.d_gradient_scale = (int64_t*)(ws + P.scale64);
  ChainPrepOp prep;
  prep.value = bio.d_value; prep.reward = bio.d_reward; prep.policy = bio.d_policy; prep.scale = bio.d_gradient_scale; prep.action = bio.d_action;
  prep.value_out = (float*)(ws + P.value); prep.reward_out = (float*)(ws + P.reward); prep.policy_out = (float*)(ws + P.policy);
  prep.scale_out = (float*)(ws + P.scale); prep.action_out = (int32_t*)(ws + P.action);
  prep.rows = (int64_t)B * steps; prep.A = pool.action_space_size;
  mzx_train_resnet_io tio;      // (its prefix is the mzx_train_fc_io of a fully connected step: csrc/mzx_train_step.h)
  memset(&tio, 0, sizeof(tio));
  tio.d_flat = io->d_flat; tio.d_observation = bio.d_observation; tio.d_action = prep.action_out;
  tio.d_target_value = prep.value_out; tio.d_target_reward = prep.reward_out; tio.d_target_policy = prep.policy_out;
  tio.d_gradient_scale = prep.scale_out; tio.d_weight = sio.d_weight;
  tio.batch = B; tio.steps = steps; tio.value_loss_weight = io->value_loss_weight; tio.per_alpha = io->per_alpha;
  tio.d_grad_flat = io->d_grad_flat; tio.d_priorities = (float*)(ws + P.priorities);
  tio.d_scratch = ws + P.scratch; tio.scratch_bytes = P.step_scratch_bytes;
  tio.d_stats = (float*)(ws + P.stats);
  mzx_optim_io oio = io->optim;
  for (int32_t i = 0; i < io->num_steps; ++i) {
    sio.call_counter = io->first_call + (uint64_t)i;
    if (const int rc = mzx_replay_sample(io->sampler, &sio, stream)) return rc;
    if (const int rc = mzx_replay_batch(io->pool, &bio, stream)) return rc;
    MZX_TRY_LAUNCH(launch<256>(prep, (stream_t)stream));
    tio.d_losses = io->d_losses + 4 * (int64_t)i;
    if (const int rc = residual ? mzx_train_resnet_step(net, &tio, stream)
                                : mzx_train_fc_step(net, reinterpret_cast<const mzx_train_fc_io*>(&tio), stream)) return rc;
    oio.t = io->optim.t + i;
    oio.first_step = i == 0 ? io->optim.first_step : 0;
    if (adam) { oio.step_size = io->h_step_size[i]; oio.bias_correction2_sqrt = io->h_bias_correction2_sqrt[i]; }
    else oio.lr = io->h_lr[i];
    MZX_TRY_LAUNCH(optim_launch(&oio, (stream_t)stream));
    if (residual)
      if (const int rc = mzx_train_resnet_commit_stats(net, tio.d_stats, io->d_flat, stream)) return rc;
    if (io->per)
      if (const int rc = mzx_replay_update_priorities(io->sampler, tio.d_priorities, sio.d_game_id, sio.d_pos, B, steps, stream)) return rc;
  }
  return mzx_net_set_weights(net, io->d_flat, net->num_params, io->d_derived, io->derived_floats, stream);
}

// ------------------------------------------------------------- natively stepped games + the round loop of a shard

int mzx_game_create(const char* kind, int32_t num_games, const uint32_t* seeds, const int32_t* observation_shape,
                    int32_t action_space_size, int32_t num_players, mzx_game** out) {
  if (!out) { set_error("mzx_game_create: null out"); return MZX_ERR_INVALID; }
  std::string err;
  mzx_game* g = game_make(kind, num_games, seeds, observation_shape, action_space_size, num_players, err);
  if (!g) { set_error("%s", err.c_str()); return MZX_ERR_INVALID; }
  *out = g;
  return MZX_OK;
}

void mzx_game_destroy(mzx_game* g) { delete g; }

int mzx_game_info(const mzx_game* g, int32_t out[8]) {
  if (!g || !out) { set_error("mzx_game_info: null"); return MZX_ERR_INVALID; }
  out[0] = g->shape[0]; out[1] = g->shape[1]; out[2] = g->shape[2]; out[3] = g->num_actions; out[4] = g->num_players;
  out[5] = g->obs_dtype; out[6] = g->reward_is_int; out[7] = g->always_all_legal;
  return MZX_OK;
}

int mzx_game_reset(mzx_game* g, const int32_t* games, int32_t count) {
  if (!g || count < 0) { set_error("mzx_game_reset: argument"); return MZX_ERR_INVALID; }
  if (!games) { g->reset(nullptr, g->num_games); return MZX_OK; }
  for (int32_t k = 0; k < count; ++k)
    if (games[k] < 0 || games[k] >= g->num_games) { set_error("mzx_game_reset: game %d out of range", games[k]); return MZX_ERR_INVALID; }
  g->reset(games, count);
  return MZX_OK;
}

int mzx_game_observe(const mzx_game* g, float* out) {
  if (!g || !out) { set_error("mzx_game_observe: null"); return MZX_ERR_INVALID; }
  g->observe(0, g->num_games, out);
  return MZX_OK;
}

int mzx_game_legal_actions(const mzx_game* g, int32_t* out) {
  if (!g || !out) { set_error("mzx_game_legal_actions: null"); return MZX_ERR_INVALID; }
  g->legal_actions(0, g->num_games, out);
  return MZX_OK;
}

int mzx_game_to_play(const mzx_game* g, int32_t* out) {
  if (!g || !out) { set_error("mzx_game_to_play: null"); return MZX_ERR_INVALID; }
  g->to_play(0, g->num_games, out);
  return MZX_OK;
}

int mzx_game_step(mzx_game* g, const int64_t* actions, const uint8_t* active, double* reward, uint8_t* done) {
  if (!g || !actions || !reward || !done) { set_error("mzx_game_step: null"); return MZX_ERR_INVALID; }
  for (int32_t k = 0; k < g->num_games; ++k)
    if ((!active || active[k]) && (actions[k] < 0 || actions[k] >= g->num_actions)) {
      set_error("mzx_game_step: action %lld of game %d outside the action space", (long long)actions[k], k);
      return MZX_ERR_INVALID;
    }
  g->step(0, g->num_games, actions, active, reward, done);
  return MZX_OK;
}

// ---- the device-resident twin of a game object (mzx_games_device.h)

int mzx_game_device_create(const mzx_game* host, mzx_game_device** out) {
  if (!host || !out) { set_error("mzx_game_device_create: null argument"); return MZX_ERR_INVALID; }
  const GameView h = host->view();
  const GameDeviceLayout L = game_device_layout(h);
  mzx_game_device* d = new (std::nothrow) mzx_game_device();
  if (!d) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  d->v = h;
  d->block_bytes = L.total;
  if (device_alloc(&d->block, L.total) != 0) {
    delete d;
    set_error("mzx_game_device_create: device allocation of %lld bytes failed", (long long)L.total);
    return MZX_ERR_RUNTIME;
  }
  game_device_point(&d->v, (char*)d->block, L);
  int rc = h.kind == 0 ? copy_h2d_blocking(d->v.seeds, h.seeds, 4 * (size_t)h.num_games)
                       : copy_h2d_blocking((void*)d->v.lines, h.lines, 4 * (size_t)h.num_lines * h.k);
  game_state_copy(d->v, h, [&](void* to, void* from, size_t bytes) { if (rc == 0) rc = copy_h2d_blocking(to, from, bytes); });
  if (rc != 0) {
    device_free(d->block);
    delete d;
    set_error("mzx_game_device_create: upload failed: %s", runtime_error_string(rc));
    return MZX_ERR_RUNTIME;
  }
  *out = d;
  return MZX_OK;
}

void mzx_game_device_destroy(mzx_game_device* d) {
  if (!d) return;
  if (d->block) device_free(d->block);
  delete d;
}

int mzx_game_device_step(mzx_game_device* d, const int64_t* d_actions, const uint8_t* d_active, double* d_reward, uint8_t* d_done,
                         void* stream) {
  if (!d || !d_actions) { set_error("mzx_game_device_step: null game or actions"); return MZX_ERR_INVALID; }
  MZX_TRY_LAUNCH(launch_waves<GAME_WAVES>(GameStepBody{d->v, d_actions, d_active, d_reward, d_done}, (stream_t)stream));
  return MZX_OK;
}

int mzx_game_device_position(const mzx_game_device* d, float* d_obs, int32_t* d_legal, int32_t* d_to_play, void* stream) {
  if (!d) { set_error("mzx_game_device_position: null game"); return MZX_ERR_INVALID; }
  if (!d_obs && !d_legal && !d_to_play) return MZX_OK;
  MZX_TRY_LAUNCH(launch_waves<GAME_WAVES>(GamePositionBody{d->v, d_obs, d_legal, d_to_play}, (stream_t)stream));
  return MZX_OK;
}

int mzx_game_device_reset(mzx_game_device* d, const int32_t* d_games, int32_t count, void* stream) {
  if (!d || count < 0) { set_error("mzx_game_device_reset: argument"); return MZX_ERR_INVALID; }
  if (!d_games) count = d->v.num_games;
  MZX_TRY_LAUNCH(launch_waves<GAME_WAVES>(GameResetBody{d->v, d_games, count}, (stream_t)stream));
  return MZX_OK;
}

int mzx_game_device_download(const mzx_game_device* d, mzx_game* host, void* stream) {
  if (!d || !host) { set_error("mzx_game_device_download: null argument"); return MZX_ERR_INVALID; }
  const GameView h = host->view();
  if (h.kind != d->v.kind || h.num_games != d->v.num_games || h.num_actions != d->v.num_actions || h.num_players != d->v.num_players ||
      h.obs_elems != d->v.obs_elems || h.rows != d->v.rows || h.cols != d->v.cols || h.k != d->v.k) {
    set_error("mzx_game_device_download: the host object is not the kind and size of game the device state was created from");
    return MZX_ERR_INVALID;
  }
  int rc = 0;
  game_state_copy(h, d->v, [&](void* to, void* from, size_t bytes) { if (rc == 0) rc = copy_d2h(to, from, bytes, (stream_t)stream); });
  const int waited = stream_sync((stream_t)stream);      // (also behind a failed copy: nothing stays in flight into the host object)
  if (rc == 0) rc = waited;
  if (rc != 0) { set_error("mzx_game_device_download: %s", runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  return MZX_OK;
}

int mzx_actor_create(const mzx_actor_config* c, mzx_actor** out) {
  if (!c || !out || !c->game || !c->search || !c->bank || !c->streams || !c->d_arena) { set_error("mzx_actor_create: missing argument"); return MZX_ERR_INVALID; }
  const mzx_game* g = c->game;
  const mzx_move& m = c->move;
  if (m.num_games != g->num_games || m.action_space_size != g->num_actions || c->max_moves < 1 ||
      !m.h_in || !m.d_in || !m.h_out || !m.d_out || !m.io.d_noise) {
    set_error("mzx_actor_create: the move block does not fit the game (%d games x %d actions) or lacks a staging block / root noise",
              g->num_games, g->num_actions);
    return MZX_ERR_INVALID;
  }
  int rc = rng_check(c->bank, c->streams, g->num_games);
  if (rc) return rc;
  mzx_actor* a = new (std::nothrow) mzx_actor();
  if (!a) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  a->game = c->game; a->search = c->search; a->bank = c->bank; a->d_arena = c->d_arena; a->arena_bytes = c->arena_bytes;
  a->move = c->move;
  a->move.add_exploration_noise = 1;
  a->B = g->num_games; a->A = g->num_actions; a->E = g->obs_elems(); a->max_moves = c->max_moves; a->first_slot = c->first_slot;
  const size_t B = (size_t)a->B, A = (size_t)a->A;
  a->streams.assign(c->streams, c->streams + B);
  a->legal.resize(B * A); a->to_play.resize(B); a->n_legal.resize(B); a->words.resize(B);
  a->cur_obs.resize(B * (size_t)a->E); a->next_obs.resize(B * (size_t)a->E);
  a->actions.resize(B); a->start.assign(B, 0);
  a->temps.assign(B, c->temperature); a->move_temps.resize(B); a->reward.resize(B); a->done.resize(B);
  a->game->reset(nullptr, a->B);
  a->game->observe(0, a->B, a->cur_obs.data());
  actor_refresh(a);
  *out = a;
  return MZX_OK;
}

void mzx_actor_destroy(mzx_actor* a) {
  if (!a) return;
  if (a->pending) (void)event_wait(a->event);
  event_destroy(a->event);
  event_destroy(a->start_event);
  stream_destroy(a->own_stream);
  if (a->d_pow) device_free(a->d_pow);
  resident_free(a);
  delete a;
}

int mzx_actor_set_device_draws(mzx_actor* a, uint64_t seed, uint64_t first_counter, double* d_temperature, int64_t* d_action) {
  if (!a) { set_error("mzx_actor_set_device_draws: null actor"); return MZX_ERR_INVALID; }
  if (a->pending) { set_error("mzx_actor_set_device_draws: a search is in flight"); return MZX_ERR_INVALID; }
  if (a->A > DRAWS_MAX_ACTIONS || a->move.tape_words < 1) {
    set_error("mzx_actor_set_device_draws: at most %d actions and at least one tape word", DRAWS_MAX_ACTIONS);
    return MZX_ERR_INVALID;
  }
  for (int k = 1; k < a->B; ++k)
    if (a->streams[k] != a->streams[0] + k) { set_error("mzx_actor_set_device_draws: the group's streams must be consecutive slots"); return MZX_ERR_INVALID; }
  const mzx_move& m = a->move;
  if (!move_in(&m).holds(d_temperature, sizeof(double) * a->B) || !move_out(&m).holds(d_action, sizeof(int64_t) * a->B)) {
    set_error("mzx_actor_set_device_draws: d_temperature must lie inside the staged input block, d_action inside the output block");
    return MZX_ERR_INVALID;
  }
  if (!m.io.d_noise || !m.io.d_tape) { set_error("mzx_actor_set_device_draws: io.d_noise / io.d_tape missing"); return MZX_ERR_INVALID; }
  a->device_draws = true; a->draw_seed = seed; a->draw_counter = first_counter;
  a->d_temperature = d_temperature; a->d_action = d_action;
  return MZX_OK;
}

int64_t mzx_actor_draw_counter(const mzx_actor* a) { return a ? (int64_t)a->draw_counter : -1; }

int mzx_actor_set_draw_counter(mzx_actor* a, uint64_t counter) {
  if (!a || !a->device_draws) { set_error("mzx_actor_set_draw_counter: not an actor on device draws"); return MZX_ERR_INVALID; }
  if (a->pending) { set_error("mzx_actor_set_draw_counter: a search is in flight"); return MZX_ERR_INVALID; }
  a->draw_counter = counter;
  return MZX_OK;
}

// ------------------------------------------------------------- resident rounds (mzx_resident.h)

int mzx_actor_set_resident(mzx_actor* a, int32_t chunk_rounds, int64_t max_log_bytes) {
  const char* who = "mzx_actor_set_resident";
  if (!a) { set_error("%s: null actor", who); return MZX_ERR_INVALID; }
  if (!a->device_draws) { set_error("%s: the group must be on device draws first (mzx_actor_set_device_draws)", who); return MZX_ERR_INVALID; }
  if (chunk_rounds < 1) { set_error("%s: chunk_rounds %d must be at least 1", who, chunk_rounds); return MZX_ERR_INVALID; }
  if (a->pending || a->round != 0) { set_error("%s: the group has played rounds already", who); return MZX_ERR_INVALID; }
  const mzx_move& m = a->move;
  const Block in = move_in(&m), out = move_out(&m);
  const size_t B = (size_t)a->B, A = (size_t)a->A, E = (size_t)a->E;
  if (!in.holds(m.io.d_observation, 4 * B * E) || !in.holds(m.io.d_legal_actions, 4 * B * A) || !in.holds(m.io.d_to_play, 4 * B) ||
      !out.holds(m.io.d_visit_counts, 4 * B * A) || !out.holds(m.io.d_root_value, 8 * B) || !out.holds(m.io.d_info, 16 * B)) {
    set_error("%s: the move's observation, legal rows and to_play must lie inside the input block, its outputs inside the output block", who);
    return MZX_ERR_INVALID;
  }
  resident_free(a);
  const bool masks = !a->game->always_all_legal;
  if (masks && a->game->view().kind != 1) { set_error("%s: a game with varying legal sets that is no board game", who); return MZX_ERR_INVALID; }
  ResidentDevice d;
  d.B = a->B; d.A = a->A; d.E = (int32_t)a->E; d.max_moves = a->max_moves; d.chunk = chunk_rounds; d.masks = masks ? 1 : 0;
  d.cap = (int64_t)a->max_moves + chunk_rounds + 1;
  const ResidentLayout L = resident_layout(d);
  if ((int64_t)L.total > max_log_bytes) {
    set_error("%s: the device log of this group takes %lld bytes (%lld rows of %d slots), more than max_log_bytes = %lld", who,
              (long long)L.total, (long long)d.cap, a->B, (long long)max_log_bytes);
    return MZX_ERR_INVALID;
  }
  mzx_actor_resident* R = new (std::nothrow) mzx_actor_resident();
  if (!R) { set_error("out of host memory"); return MZX_ERR_RUNTIME; }
  a->resident = R;
  int rc = mzx_game_device_create(a->game, &R->game);
  if (rc) { resident_free(a); return rc; }
  if (device_alloc(&R->block, L.total) != 0) {
    R->block = nullptr;
    resident_free(a);
    set_error("%s: device allocation of %lld bytes failed", who, (long long)L.total);
    return MZX_ERR_RUNTIME;
  }
  R->block_bytes = R->stats[5] = (int64_t)L.total;
  R->max_log_bytes = max_log_bytes;
  d.game = R->game->v;
  resident_point(&d, (char*)R->block, L);
  d.in_obs = (float*)m.io.d_observation; d.in_legal = (int32_t*)m.io.d_legal_actions; d.in_to_play = (int32_t*)m.io.d_to_play;
  d.in_temperature = a->d_temperature;
  d.visits = m.io.d_visit_counts; d.root_value = m.io.d_root_value; d.action = a->d_action; d.info = m.io.d_info;
  R->d = d;
  R->h_ctrl.assign(RESIDENT_CTRL_WORDS + (size_t)chunk_rounds * B, 0);
  return MZX_OK;
}

int mzx_actor_resident_stats(const mzx_actor* a, int64_t out[8]) {
  if (!a || !out) { set_error("mzx_actor_resident_stats: null"); return MZX_ERR_INVALID; }
  if (!a->resident) { set_error("mzx_actor_resident_stats: not a resident group"); return MZX_ERR_INVALID; }
  for (int k = 0; k < 8; ++k) out[k] = a->resident->stats[k];
  return MZX_OK;
}

int mzx_selfplay_rounds(mzx_actor* const* groups, int32_t num_groups, mzx_rounds* io, void* stream) {
  if (!groups || num_groups < 1 || !io) { set_error("mzx_selfplay_rounds: missing argument"); return MZX_ERR_INVALID; }
  for (int k = 0; k < num_groups; ++k)
    if (!groups[k]) { set_error("mzx_selfplay_rounds: null group"); return MZX_ERR_INVALID; }
  int resident_groups = 0;
  for (int k = 0; k < num_groups; ++k) resident_groups += groups[k]->resident ? 1 : 0;
  if (resident_groups != 0 && resident_groups != num_groups) {
    set_error("mzx_selfplay_rounds: %d of the call's %d groups are resident (mzx_actor_set_resident): all or none", resident_groups, num_groups);
    return MZX_ERR_INVALID;
  }
  const double t_call = actor_now();
  for (double& x : io->phase_seconds) x = 0.0;
  const RoundsArgs args{io->phase_seconds, io->temperature, io->temperature_threshold, io->pow_table, io->table_stride,
                        io->table_temperatures, io->num_temperatures, io->retry, io->retry_ctx};
  int64_t finished = 0, rounds = 0, searches = 0, sequence = io->sequence;
  double search_seconds = 0.0;
  int rc = MZX_OK;
  // Streams: the first group searches on the caller's stream, every further group on a stream of its own, ordered behind
  // whatever the caller queued before this call (a weight upload).  Half a shard of a small network fills half the chip
  // (C2: 2048 trees = two waves per CU), and such a search is latency-bound -- it takes as long as the whole shard's -- so
  // the two groups' searches must run SIDE BY SIDE, not one behind the other, for the pipelining to pay.  Every search is
  // waited for on the host before its results are read and nothing is in flight when the call returns.
  std::vector<void*> streams((size_t)num_groups, stream);
  for (int k = 1; k < num_groups && rc == MZX_OK; ++k) {
    mzx_actor* a = groups[k];
    if (tune(TUNE_ROUNDS_STREAMS) == 0) break;
    if (!a->own_stream && stream_create(&a->own_stream) != 0) { a->own_stream = nullptr; continue; }
    if (!a->own_stream) continue;          // (a build without streams: the caller's)
    if (event_record(&a->start_event, (stream_t)stream) != 0 || stream_wait_event((stream_t)a->own_stream, a->start_event) != 0) {
      set_error("mzx_selfplay_rounds: ordering the group's stream behind the caller's failed");
      rc = MZX_ERR_RUNTIME;
      break;
    }
    streams[(size_t)k] = a->own_stream;
  }
  for (int k = 0; k < num_groups && rc == MZX_OK; ++k) rc = actor_upload_pow(groups[k], args);
  if (rc == MZX_OK && resident_groups) {
    for (int k = 0; k < num_groups; ++k)
      if (groups[k]->pending) { set_error("mzx_selfplay_rounds: a search is in flight for resident group %d", k); rc = MZX_ERR_INVALID; }
    if (rc == MZX_OK) rc = resident_rounds(groups, num_groups, io, args, streams, &finished, &rounds, &searches, &sequence);
  } else if (rc == MZX_OK) {
    rc = actor_rounds(groups, num_groups, io, args, streams, &finished, &rounds, &searches, &sequence, &search_seconds);
  }
  if (rc != MZX_OK) {          // nothing stays in flight behind a failure
    for (int k = 0; k < num_groups; ++k) (void)stream_sync((stream_t)streams[(size_t)k]);
    for (int k = 0; k < num_groups; ++k) groups[k]->pending = false;
  }
  io->phase_seconds[5] = (actor_now() - t_call) - (io->phase_seconds[0] + io->phase_seconds[1] + io->phase_seconds[2] +
                                                   io->phase_seconds[3] + io->phase_seconds[4]);
  if (resident_groups) search_seconds = io->phase_seconds[0] + io->phase_seconds[1];
  io->rounds = rounds; io->games = finished; io->searches = searches; io->search_seconds = search_seconds; io->sequence = sequence;
  return rc;
}

// ------------------------------------------------------------- the device hand-off of a resident group (mzx_resident.h)

int mzx_actor_set_device_handoff(mzx_actor* a, int32_t on) {
  const char* who = "mzx_actor_set_device_handoff";
  if (!a) { set_error("%s: null actor", who); return MZX_ERR_INVALID; }
  if (!a->resident) { set_error("%s: not a resident group (mzx_actor_set_resident first)", who); return MZX_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(a->finished_lock);
  if (!a->finished.empty() || !a->resident->queued.empty()) {
    set_error("%s: the group has finished games pending: take them first", who);
    return MZX_ERR_INVALID;
  }
  a->resident->handoff = on != 0;
  return MZX_OK;
}

static int handoff_group(const char* who, const mzx_actor* a) {
  if (!a) { set_error("%s: null actor", who); return MZX_ERR_INVALID; }
  if (!a->resident || !a->resident->handoff) { set_error("%s: not a group on the device hand-off (mzx_actor_set_device_handoff)", who); return MZX_ERR_INVALID; }
  return MZX_OK;
}

int mzx_actor_finished_device(mzx_actor* a, int64_t before_sequence, int64_t out[2]) {
  const int rc = handoff_group("mzx_actor_finished_device", a);
  if (rc) return rc;
  if (!out) { set_error("mzx_actor_finished_device: null"); return MZX_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(a->finished_lock);
  out[0] = out[1] = 0;
  for (const mzx_actor_piece* p : a->resident->queued) {
    if (before_sequence >= 0 && !p->seq.empty() && p->seq[0] >= before_sequence) break;
    out[0] += 1; out[1] += p->games;
  }
  return MZX_OK;
}

int mzx_actor_take_device(mzx_actor* a, int64_t before_sequence, int32_t max_pieces, int64_t max_games, int64_t* piece_info,
                          int32_t* slot, int32_t* length, int64_t* sequence, int64_t out[2]) {
  const int rc = handoff_group("mzx_actor_take_device", a);
  if (rc) return rc;
  if (max_pieces < 0 || max_games < 0 || !out || (max_pieces > 0 && !piece_info) || (max_games > 0 && (!slot || !length || !sequence))) {
    set_error("mzx_actor_take_device: missing buffer or negative capacity");
    return MZX_ERR_INVALID;
  }
  mzx_actor_resident* R = a->resident;
  std::lock_guard<std::mutex> lk(a->finished_lock);
  int64_t pieces = 0, games = 0;
  while (!R->queued.empty() && pieces < max_pieces) {
    mzx_actor_piece* p = R->queued.front();
    if (before_sequence >= 0 && !p->seq.empty() && p->seq[0] >= before_sequence) break;
    if (games + p->games > max_games) break;
    const char* base = (const char*)p->buf;
    const int64_t row[MZX_PIECE_INFO_WORDS] = {
        p->token, p->games, p->rows0, p->mask ? 1 : 0, (int64_t)(intptr_t)(base + p->o_len), (int64_t)(intptr_t)(base + p->o_src1),
        (int64_t)(intptr_t)(base + p->o_src0), (int64_t)(intptr_t)(base + p->o_obs), (int64_t)(intptr_t)(base + p->o_act),
        (int64_t)(intptr_t)(base + p->o_rew), (int64_t)(intptr_t)(base + p->o_tp), (int64_t)(intptr_t)(base + p->o_vis),
        (int64_t)(intptr_t)(base + p->o_val), p->mask ? (int64_t)(intptr_t)(base + p->o_mask) : 0, p->bytes, 0};
    memcpy(piece_info + MZX_PIECE_INFO_WORDS * pieces, row, sizeof(row));
    memcpy(slot + games, p->slot.data(), sizeof(int32_t) * (size_t)p->games);
    memcpy(length + games, p->n.data(), sizeof(int32_t) * (size_t)p->games);
    memcpy(sequence + games, p->seq.data(), sizeof(int64_t) * (size_t)p->games);
    p->state = mzx_actor_piece::TAKEN;
    R->queued.pop_front();
    pieces += 1; games += p->games;
  }
  out[0] = pieces; out[1] = games;
  return MZX_OK;
}

int mzx_actor_download_device(mzx_actor* a, int64_t token, float* observations, int64_t* actions, double* rewards, int64_t* to_play,
                              int32_t* visit_counts, double* root_values, uint8_t* legal_mask, void* stream) {
  const char* who = "mzx_actor_download_device";
  if (!a || !a->resident) { set_error("%s: not a resident group", who); return MZX_ERR_INVALID; }
  const mzx_actor_piece* p;
  {
    std::lock_guard<std::mutex> lk(a->finished_lock);
    p = resident_piece_find(a->resident, token, mzx_actor_piece::TAKEN);
  }
  if (!p) { set_error("%s: no piece with token %lld is taken and unreleased", who, (long long)token); return MZX_ERR_INVALID; }
  const size_t A = (size_t)a->A, E = (size_t)a->E, n1 = (size_t)(p->rows0 + p->games), n0 = (size_t)p->rows0;
  if (legal_mask && !p->mask) { set_error("%s: the piece carries no legal mask", who); return MZX_ERR_INVALID; }
  const char* base = (const char*)p->buf;
  struct { void* dst; const void* src; size_t bytes; } copies[7] = {
      {observations, base + p->o_obs, 4 * n1 * E}, {actions, base + p->o_act, 8 * n1}, {rewards, base + p->o_rew, 8 * n1},
      {to_play, base + p->o_tp, 8 * n1}, {visit_counts, base + p->o_vis, 4 * n0 * A}, {root_values, base + p->o_val, 8 * n0},
      {legal_mask, base + p->o_mask, n0 * A}};
  int rc = 0;
  for (const auto& cp : copies)
    if (cp.dst && cp.bytes && rc == 0) rc = copy_d2h(cp.dst, cp.src, cp.bytes, (stream_t)stream);
  const int waited = stream_sync((stream_t)stream);      // (also behind a failed copy: nothing stays in flight into the host arrays)
  if (rc == 0) rc = waited;
  if (rc) { set_error("%s: %s", who, runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  return MZX_OK;
}

int mzx_actor_release_device(mzx_actor* a, int64_t token, void* stream) {
  const char* who = "mzx_actor_release_device";
  if (!a || !a->resident) { set_error("%s: not a resident group", who); return MZX_ERR_INVALID; }
  std::lock_guard<std::mutex> lk(a->finished_lock);
  mzx_actor_piece* p = resident_piece_find(a->resident, token, mzx_actor_piece::TAKEN);
  if (!p) { set_error("%s: no piece with token %lld is taken and unreleased", who, (long long)token); return MZX_ERR_INVALID; }
  const int rc = event_record(&p->event, (stream_t)stream);
  if (rc) { set_error("%s: event record failed: %s", who, runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  p->event_pending = true;
  p->state = mzx_actor_piece::FREE;
  return MZX_OK;
}

static int no_handoff_group(const char* who, const mzx_actor* a) {
  if (a && a->resident && a->resident->handoff) {
    set_error("%s: the group is on the device hand-off: its games are taken with mzx_actor_take_device", who);
    return MZX_ERR_INVALID;
  }
  return MZX_OK;
}

int mzx_actor_finished(mzx_actor* a, int64_t before_sequence, int64_t out[3]) {
  if (!a || !out) { set_error("mzx_actor_finished: null"); return MZX_ERR_INVALID; }
  if (no_handoff_group("mzx_actor_finished", a)) return MZX_ERR_INVALID;
  std::lock_guard<std::mutex> lk(a->finished_lock);
  out[0] = out[1] = out[2] = 0;
  for (const mzx_actor::Batch& b : a->finished) {
    if (before_sequence >= 0 && !b.seq.empty() && b.seq[0] >= before_sequence) break;
    out[0] += (int64_t)b.slot.size(); out[1] += (int64_t)b.val.size();
    if (!b.mask.empty()) out[2] = 1;
  }
  return MZX_OK;
}

int mzx_actor_take(mzx_actor* a, int64_t before_sequence, int32_t* slot, int32_t* length, int64_t* sequence, float* observations,
                   int64_t* actions, double* rewards, int64_t* to_play, int32_t* visit_counts, double* root_values,
                   uint8_t* legal_mask, int32_t* any_illegal) {
  if (!a || !slot || !length || !sequence || !observations || !actions || !rewards || !to_play || !visit_counts || !root_values) {
    set_error("mzx_actor_take: missing buffer");
    return MZX_ERR_INVALID;
  }
  if (no_handoff_group("mzx_actor_take", a)) return MZX_ERR_INVALID;
  // the batches to hand out leave the queue under its lock (a rounds call on another thread may be appending); the copies
  // run outside it
  std::deque<mzx_actor::Batch> mine;
  {
    std::lock_guard<std::mutex> lk(a->finished_lock);
    while (!a->finished.empty()) {
      mzx_actor::Batch& b = a->finished.front();
      if (before_sequence >= 0 && !b.seq.empty() && b.seq[0] >= before_sequence) break;
      if (!b.mask.empty() && !legal_mask) { set_error("mzx_actor_take: games with restricted legal sets need the legal_mask buffer"); return MZX_ERR_INVALID; }
      mine.push_back(std::move(b));
      a->finished.pop_front();
    }
  }
  const size_t A = (size_t)a->A, E = (size_t)a->E;
  size_t g = 0, q1 = 0, q0 = 0;
  int32_t illegal = 0;
  for (const mzx_actor::Batch& b : mine) {
    const size_t k = b.slot.size(), n1 = b.act.size(), n0 = b.val.size();
    memcpy(slot + g, b.slot.data(), sizeof(int32_t) * k);
    memcpy(length + g, b.n.data(), sizeof(int32_t) * k);
    memcpy(sequence + g, b.seq.data(), sizeof(int64_t) * k);
    memcpy(observations + q1 * E, b.obs.data(), sizeof(float) * n1 * E);
    memcpy(actions + q1, b.act.data(), sizeof(int64_t) * n1);
    memcpy(rewards + q1, b.rew.data(), sizeof(double) * n1);
    memcpy(to_play + q1, b.tp.data(), sizeof(int64_t) * n1);
    memcpy(visit_counts + q0 * A, b.vis.data(), sizeof(int32_t) * n0 * A);
    memcpy(root_values + q0, b.val.data(), sizeof(double) * n0);
    if (legal_mask) {
      if (b.mask.empty()) memset(legal_mask + q0 * A, 1, n0 * A);
      else { memcpy(legal_mask + q0 * A, b.mask.data(), n0 * A); illegal = 1; }
    }
    g += k; q1 += n1; q0 += n0;
  }
  if (any_illegal) *any_illegal = illegal;
  return MZX_OK;
}

}  // extern "C"
