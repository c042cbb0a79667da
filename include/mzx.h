/*
 * mzx.h -- C ABI of the MI355X-native MuZero self-play hot path (libmzx.so).
 *
 * The reference (werner-duvaud/muzero-general) has no FFI: its boundary for this
 * path is the duck-typed Python surface of models.py / self_play.py.  Every
 * entry point below names the reference interface it stands behind
 * (file:line relative to /root/reference); the Python host package
 * (muzero-general_amd/mzx) binds them with ctypes and re-exposes the reference's
 * own names (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain C types only; every `d_*` pointer is a DEVICE pointer (e.g.
 *     torch.Tensor.data_ptr()); `h_*` pointers are host pointers read during
 *     the call.  The library never allocates or frees device memory: the
 *     caller owns every buffer (sizes via the *_bytes / *_floats queries).
 *   - `stream` is a hipStream_t (0 = default stream).  Calls only ENQUEUE work
 *     on it; they never synchronise.
 *   - return value: MZX_OK or a negative MZX_ERR_* code; mzx_last_error() gives
 *     the message of the calling thread's last failure.
 *   - handles are host-side descriptors; one handle may be used by one thread
 *     at a time (the reference runs one actor per process, self_play.py:11-29).
 */
#ifndef MZX_H
#define MZX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZX_ABI_VERSION 8

#define MZX_OK 0
#define MZX_ERR_INVALID (-1)      /* bad argument / unsupported configuration */
#define MZX_ERR_RUNTIME (-2)      /* HIP runtime error */
#define MZX_ERR_WORKSPACE (-3)    /* caller-provided buffer too small */

#define MZX_MAX_LAYERS 8          /* hidden layers per MLP */

int mzx_abi_version(void);
const char* mzx_last_error(void);
/* 1 if the library was built for the GPU (always, for libmzx.so). */
int mzx_is_device_build(void);

/* ------------------------------------------------------------------------- *
 * Tuning: the library's routing / launch-shape choices as ONE process-wide table of named integers
 * (csrc/mzx_tuning.h), in place of environment variables.  No entry changes WHAT is computed (the reference
 * has no counterpart: it has one code path); the defaults are the measured best, tests
 * and bench.py move them for A/B runs.  Set a value before the calls it should affect, from the calling thread.
 *   rb_heads       head MLP levels of the streamed engine: 0 one launch per Linear layer, 2 one grouped launch per level
 *   rb_tail        1: per-plane scaling / small 1x1 head convolutions run inside the tower launch
 *   rb_tower_t     > 0: samples per tower workgroup (0: cost model)
 *   row_split_min  per-simulation launches: two half-shards on two HIP streams from this many trees (0: never)
 *   wide_towers    1: wide residual networks that would also fit the LDS-resident whole-search kernel search on the
 *                  tower arithmetic at EVERY shard size (a tree's result must not depend on the shard it is searched
 *                  in); 0: mzx::rz_search_kernel (the A/B)
 *   rt_search      the tower whole-search kernel (every simulation in one launch): -1 automatic, 0 never, 1 whenever
 *                  the network fits;  rt_trees > 0: trees per workgroup;  rt_waves 4 | 8: waves per workgroup (0: cost
 *                  model);  rt_max_trees: largest shard routed to it;  rt_dbg: timing knock-outs (wrong results);
 *                  rt_short 1 | 0: waves of a row group one tile short skip that tile's products (0: A/B, same trees)
 *   rounds_streams mzx_selfplay_rounds: 1 = every slot group behind the first searches on a stream of its own (two half-shard
 *                  searches of a small network run side by side); 0 = all on the caller's stream (the A/B)
 *   wave_select    per-simulation launches, more than 16 actions: 1 = the selection walk by a wavefront per tree (lane l scores
 *                  child slots l, l + 64, ...), 0 = by a 16-lane row per tree (the A/B); the same walks either way
 * mzx_tuning_set / _get return MZX_ERR_INVALID for an unknown name or a value out of range; mzx_tuning_name /
 * _help enumerate the table (NULL past its end).
 * ------------------------------------------------------------------------- */
int mzx_tuning_set(const char* name, int32_t value);
int mzx_tuning_get(const char* name, int32_t* value /* nullable */, int32_t* default_value /* nullable */);
const char* mzx_tuning_name(int32_t index);
const char* mzx_tuning_help(int32_t index);

/* ------------------------------------------------------------------------- *
 * Network: replaces models.MuZeroNetwork(config) -- models.py:7-41 (factory),
 * :80-195 (MuZeroFullyConnectedNetwork), :436-623 (MuZeroResidualNetwork).
 * Field names are the MuZeroConfig attributes the factory reads.
 * ------------------------------------------------------------------------- */
typedef struct mzx_net_config {
  int32_t network;               /* 0 = "fullyconnected", 1 = "resnet" */
  int32_t observation_shape[3];  /* (channels, height, width) */
  int32_t stacked_observations;
  int32_t action_space_size;     /* len(config.action_space) */
  int32_t support_size;
  /* fullyconnected (models.py:80-126) */
  int32_t encoding_size;
  int32_t n_fc_representation_layers, fc_representation_layers[MZX_MAX_LAYERS];
  int32_t n_fc_dynamics_layers, fc_dynamics_layers[MZX_MAX_LAYERS];
  int32_t n_fc_reward_layers, fc_reward_layers[MZX_MAX_LAYERS];
  int32_t n_fc_value_layers, fc_value_layers[MZX_MAX_LAYERS];
  int32_t n_fc_policy_layers, fc_policy_layers[MZX_MAX_LAYERS];
  /* resnet (models.py:436-520) */
  int32_t downsample;            /* 0 = False, 1 = "resnet" (DownSample, models.py:233-275), 2 = "CNN" (DownsampleCNN, :278-297) */
  int32_t blocks, channels;
  int32_t reduced_channels_reward, reduced_channels_value, reduced_channels_policy;
  int32_t n_resnet_fc_reward_layers, resnet_fc_reward_layers[MZX_MAX_LAYERS];
  int32_t n_resnet_fc_value_layers, resnet_fc_value_layers[MZX_MAX_LAYERS];
  int32_t n_resnet_fc_policy_layers, resnet_fc_policy_layers[MZX_MAX_LAYERS];
} mzx_net_config;

typedef struct mzx_net mzx_net;

/* models.MuZeroNetwork.__new__ (models.py:7-41): validates, builds the operator program. */
int mzx_net_create(const mzx_net_config* cfg, mzx_net** out);
void mzx_net_destroy(mzx_net* net);

/* The flat weight buffer = every floating-point tensor of the reference
 * state_dict (AbstractNetwork.get_weights, models.py:69-70) concatenated in
 * state_dict order (BatchNorm running stats included, num_batches_tracked
 * skipped).  This one buffer is what RCCL broadcasts. */
int32_t mzx_net_num_tensors(const mzx_net* net);
int64_t mzx_net_num_params(const mzx_net* net);
/* i-th tensor: reference state_dict key (with the ".module." infix), offset/numel
 * in floats, up to 4 dims (unused dims = 0). */
int mzx_net_tensor_info(const mzx_net* net, int32_t i, char* name, int32_t name_cap,
                        int64_t* offset, int64_t* numel, int32_t dims[4]);
int64_t mzx_net_hidden_size(const mzx_net* net);     /* floats per encoded state */
int64_t mzx_net_input_size(const mzx_net* net);      /* floats per stacked observation */
int64_t mzx_net_derived_floats(const mzx_net* net);  /* folded-BatchNorm buffer size */
int64_t mzx_net_workspace_floats(const mzx_net* net, int32_t max_batch);
/* 2 x multiply-accumulates of one sample's initial_inference (recurrent = 0) or
 * recurrent_inference (1): convolutions and linear layers, as the reference's modules count. */
int64_t mzx_net_flops(const mzx_net* net, int32_t recurrent);

/* AbstractNetwork.set_weights (models.py:72-73): bind the flat device buffer
 * (kept alive by the caller) and derive folded BatchNorm terms into d_derived.
 * d_derived and every d_workspace / d_scratch below may come straight from hipMalloc: no call reads a word of them
 * that it (or, for d_derived, this call) has not written; the padding words between the regions of d_derived are
 * never read and keep whatever they held.  tests/poison_cases.py holds every entry to this on both builds. */
int mzx_net_set_weights(mzx_net* net, const float* d_flat, int64_t n_floats,
                        float* d_derived, int64_t derived_floats, void* stream);

/* Residual networks run on the fused MFMA engine (one launch per inference, activations
 * resident in LDS) where the configuration allows it.  mzx_net_fused_supported: bit 0 =
 * initial_inference, bit 1 = recurrent_inference.  mzx_net_set_mode(0) forces one kernel per
 * operator (the correctness reference of the tuned engine), 1 (default) re-enables it. */
int mzx_net_fused_supported(const mzx_net* net);
int mzx_net_set_mode(mzx_net* net, int32_t mode);

/* Residual networks the fused engine cannot hold in LDS (reference games/gomoku.py:56-64 -- 128 channels x 6
 * blocks on 11 x 11 -- and games/atari.py:61-69 -- 256 channels x 16 blocks, 256-wide heads; models.py:436-623)
 * run on the STREAMED MFMA engine: one FP32-MFMA implicit-GEMM launch per convolution / Linear layer over the
 * whole batch.  mzx_net_streamed_supported: bit 0 = initial_inference, bit 1 = recurrent_inference run there
 * by default (mode 0 still forces one element kernel per operator; mzx_net_set_mode(3) routes EVERY residual
 * program there, fused-capable ones included -- the A/B and parity knob; 4 = as 3 and 5 = as 1, but the streamed
 * engine launches every layer on its own, no towers).  mzx_net_streamed_plan: the workgroup tiling of
 * operator `op`: {kind, in_layout, out_layout, res_layout, taps, stride, cin, cout, hin, win, hout, wout, T, th,
 * tw, tiles_x, tiles_y, PH, PW, chunks per phase, phases, rows, row tiles, LDS bytes}. */
int mzx_net_streamed_supported(const mzx_net* net);
int mzx_net_streamed_plan(const mzx_net* net, int32_t recurrent, int32_t op, int32_t out[24]);
/* The launch shape the streamed engine picks for GEMM operator `op` at `batch` samples (small batches take fewer samples
 * per workgroup, split the column tiles over more workgroups and use fewer channel phases): {T, rows, row tiles, LDS
 * bytes, column tiles per workgroup, column splits, column tiles per wave, waves along N, waves along M, row tiles per
 * wave, row groups (grid.x), chunks per phase, phases, LDS floats per cell, column tiles, 16-channel chunks per tap}. */
int mzx_net_streamed_shape(const mzx_net* net, int32_t recurrent, int32_t op, int32_t batch, int32_t out[16]);
/* TOWERS: runs of stride-1 3x3 convolutions of one width (the representation / dynamics / prediction trunks,
 * models.py:300-433) run as ONE launch of rb_tower_kernel with the activations resident in LDS, updated in place
 * (mzx_net_set_mode(4) / (5): layer by layer instead, the A/B).  Tower `index` of the program at `batch` samples:
 * {first operator, operators, channels, H, W, samples per workgroup, row tiles per wave, column tiles per wave, waves
 * along M, waves along N, LDS bytes, workgroups (0: at this batch the tower's shape would waste more than a fifth of the
 * MFMA rows and its layers launch one by one), operators directly behind the tower that run INSIDE its launch on the
 * LDS-resident output (the per-plane min-max scaling, 1x1 head convolutions with few output channels: the tower's
 * output then never reaches memory), 0, 0, 0}; an error when the program has no such tower.  The operators of a
 * tower are not launched one by one (mzx_net_streamed_shape still describes what the layer-by-layer path would do). */
int mzx_net_streamed_tower(const mzx_net* net, int32_t recurrent, int32_t index, int32_t batch, int32_t out[16]);
/* HEADS: the Linear chains behind the small 1x1 head convolutions (dynamics fc, prediction fc_value / fc_policy,
 * models.py:379-433), when their tower runs with its tail, leave the one-launch-per-layer path: by default the k-th
 * layers of all chains run as slices of ONE rb_gemm_multi_kernel launch per level (tuning "rb_heads" = 2; the layer
 * kernel's own body and shapes: the same bits); "rb_heads" = 0: one rb_gemm_kernel launch per layer.  out = {[0] Linear operators covered at `batch` samples, [1] chains, [2..13] their operator indices,
 * [14] their levels inside their chains (2 bits each, operator k at bits 2k), [15] the mode in effect}; all zero when
 * off or when no chain qualifies. */
int mzx_net_streamed_heads(const mzx_net* net, int32_t recurrent, int32_t batch, int32_t out[16]);
/* The row-per-tree search runs large shards as two half-shards on two HIP streams (csrc/mzx_row_search.h; from 1024
 * trees, and only when both halves keep the channel groups -- the summation order -- of the undivided launch):
 * out = {trees of the first half, trees of the second half}; {batch, 0} when a shard of `batch` trees runs undivided.
 * recurrent_inference is then launched at THESE batch sizes (tests / bench.py derive the kernel instantiations a
 * workload launches from it, host-side). */
int mzx_net_streamed_split(const mzx_net* net, int32_t batch, int32_t out[2]);
/* Floats per sample of the output tensor of operator `op` (what mzx_net_debug_prefix copies out for a prefix ending
 * there); 0 for an unknown operator. */
int64_t mzx_net_operator_out_floats(const mzx_net* net, int32_t recurrent, int32_t op);

/* initial_inference(observation) (models.py:172-190 / :601-618).
 * d_observation [batch][input_size]; outputs value_logits [batch][2s+1],
 * policy_logits [batch][A], hidden [batch][hidden_size].  The reward of the
 * root is log(one-hot at the support centre), i.e. scalar 0 -- d_reward_logits
 * (nullable) is filled with -inf / 0 accordingly. */
int mzx_net_initial_inference(mzx_net* net, const float* d_observation, int32_t batch,
                              float* d_value_logits, float* d_reward_logits,
                              float* d_policy_logits, float* d_hidden,
                              float* d_workspace, int64_t workspace_floats, void* stream);

/* recurrent_inference(encoded_state, action) (models.py:192-195 / :620-623). */
int mzx_net_recurrent_inference(mzx_net* net, const float* d_hidden, const int32_t* d_action,
                                int32_t batch, float* d_value_logits, float* d_reward_logits,
                                float* d_policy_logits, float* d_next_hidden,
                                float* d_workspace, int64_t workspace_floats, void* stream);

/* Diagnostics (parity bisection, no reference counterpart): run the first n_ops operators of
 * initial_inference (recurrent = 0) or recurrent_inference (1) on the per-operator (fused = 0)
 * or fused (1) engine and copy the LAST operator's output tensor, dense per sample, to d_out.
 * fused = 2: run the whole fused program and write workgroup 0's shader-clock stamps (uint64: after
 * staging, after the input load, after every operator, at the end) to d_out instead.
 * d_scratch: (hidden_size + 2 * (2 * support_size + 1) + action_space_size) * batch floats. */
int mzx_net_num_operators(const mzx_net* net, int32_t recurrent);
/* Schedule of the fused residual engine: slot_of_op[k] = slot (barrier interval) operator k of the program
 * runs in, -1 for operators outside the fused part (down-sampling stem); operators sharing a slot have no
 * data dependence and run concurrently on disjoint wave teams.  Returns the number of slots, 0 if the
 * program is not fused.  `cap` = entries available in slot_of_op. */
int mzx_net_fused_schedule(const mzx_net* net, int32_t recurrent, int32_t* slot_of_op, int32_t cap);
int mzx_net_debug_prefix(mzx_net* net, int32_t recurrent, int32_t fused, int32_t n_ops, const float* d_input,
                         const int32_t* d_action, int32_t batch, float* d_out, int64_t out_floats,
                         float* d_scratch, int64_t scratch_floats, float* d_workspace, int64_t workspace_floats,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * Batched search: replaces MCTS(config).run(...) -- self_play.py:249-430 -- for
 * num_trees independent roots at once (the reference runs one).
 * ------------------------------------------------------------------------- */
typedef struct mzx_search_config {
  int32_t num_trees;           /* B parallel roots (one per game of the shard) */
  int32_t num_simulations;     /* config.num_simulations */
  int32_t action_space_size;   /* len(config.action_space) */
  int32_t num_players;         /* len(config.players): 1 or 2 */
  int32_t support_size;        /* config.support_size */
  int32_t tape_words;          /* raw MT19937 words per tree for argmax tie draws */
  double discount;             /* config.discount */
  double root_exploration_fraction;
  /* host tables, entries 0..num_simulations (index = parent visit count), built
   * by the caller with the language's own math library so that they are the
   * reference's values bit for bit (self_play.py:384-391):
   *   h_pb_c_table[n] = log((n + pb_c_base + 1) / pb_c_base) + pb_c_init
   *   h_sqrt_table[n] = sqrt(n) */
  const double* h_pb_c_table;
  const double* h_sqrt_table;
} mzx_search_config;

typedef struct mzx_search mzx_search;

int mzx_search_create(const mzx_search_config* cfg, mzx_net* net /* nullable: lock-step only */,
                      mzx_search** out);
void mzx_search_destroy(mzx_search* s);
/* Device memory the caller must provide as `d_arena` (trees + per-node hidden
 * states + per-simulation scratch + network workspace).  The arena is scratch: its contents need
 * NOT persist between calls (only mzx_search_dump / the lock-step calls read what the preceding
 * call of the same handle left there); the pb_c / sqrt tables live in a small device buffer owned
 * by the handle (allocated on the device current at mzx_search_create, freed by destroy). */
int64_t mzx_search_arena_bytes(const mzx_search* s);

/* Per-move inputs / outputs (all device pointers, all [num_trees] leading). */
typedef struct mzx_search_io {
  const float* d_observation;    /* [B][input_size] stacked observations (self_play.py:138-140) */
  const int32_t* d_legal_actions;/* [B][A] game.legal_actions() in the game's order, padded with -1 */
  const int32_t* d_to_play;      /* [B] game.to_play() */
  const double* d_noise;         /* [B][A] Dirichlet sample per root child slot; NULL = no exploration noise */
  const uint32_t* d_tape;        /* [B][tape_words] raw MT19937 words following the Dirichlet draw */
  int32_t* d_visit_counts;       /* out [B][A] root child visit counts by action (0 if not a child) */
  double* d_root_value;          /* out [B] root.value() */
  double* d_root_predicted_value;/* out [B] support_to_scalar(initial value head) */
  int32_t* d_info;               /* out [B][4]: max_tree_depth, flags (1 tape overflow, 2 node overflow),
                                    tape words consumed, sum of leaf depths */
} mzx_search_io;

/* MCTS.run for B roots: initial_inference, root expansion (+noise), then
 * num_simulations x {select, recurrent_inference, expand, backpropagate}. */
int mzx_search_run(mzx_search* s, const mzx_search_io* io, void* d_arena, int64_t arena_bytes, void* stream);

/* MCTS.run(..., override_root_with=root) (self_play.py:275-277) for roots the caller expanded itself,
 * as diagnose_model.py:57-74 does after a recurrent_inference: d_root_hidden [B][hidden_size],
 * d_root_priors [B][A] (binary64 Node.prior of the root's children in slot order = order of
 * io->d_legal_actions), d_root_reward [B] (Node.reward).  io->d_observation is not read and
 * io->d_root_predicted_value not written (the reference reports None).  Exploration noise, the
 * simulations and the outputs are those of mzx_search_run, on the same kernels: the residual whole-search kernels /
 * streamed engine read the given roots from the arena, the fully connected whole-search kernel (fc2_search_kernel)
 * takes them as launch arguments in place of its initial_inference. */
int mzx_search_run_from_roots(mzx_search* s, const mzx_search_io* io, const float* d_root_hidden,
                              const double* d_root_priors, const double* d_root_reward, void* d_arena,
                              int64_t arena_bytes, void* stream);

/* Which implementation mzx_search_run uses, a set of flags:
 *   1  whole-search kernel: every simulation of the move in one launch.  mzx_search_fused_supported
 *      returns 1 for the LDS-resident fully connected kernel, 2 for the residual-network kernel
 *      (trees in the arena, network on the fused MFMA engine), 3 for networks that run layer by layer on
 *      the streamed MFMA engine (per simulation: a 16-lane row per tree selects, one launch per layer,
 *      a row per tree expands and back-propagates; csrc/mzx_row_search.h), 0 if none applies;
 *      0 = generic path (select / network / expand+backpropagate launches per simulation, one thread per tree)
 *   2  (fused) also export the finished trees to the arena so mzx_search_dump works
 *   4  (fused) force the LDS-weight engine even when a register-resident
 *      specialisation matches the network shape
 *   8  cycle profile: phase cycle counters are left in the network-workspace region of the
 *      arena (mzx_search_arena_offsets): [tree][16] for the fully connected kernel (a
 *      separate profiling instantiation), [workgroup][8] for the residual kernel
 *  16  (fully connected whole-search kernel) run the first-generation kernel (per-level UCB evaluation,
 *      csrc/mzx_fused_fc.h) instead of the cached-prior-score kernel (csrc/mzx_fused_fc2.h): A/B measurements
 * Default: 1 when supported, else 0. */
int mzx_search_fused_supported(const mzx_search* s);
/* Name of the search kernel the last mzx_search_run of this handle launched ("" before the first run): which of the
 * whole-search kernels a configuration is routed to is decided per launch (network family, board size, LDS fit). */
const char* mzx_search_kernel_name(const mzx_search* s);
int mzx_search_set_mode(mzx_search* s, int32_t mode);
/* What the NEXT mzx_search_run (or mzx_search_run_continued) of this handle would launch (host-side, no GPU): out[0] = 0 the generic path, 1
 * mzx::rz_search_kernel or one of its small-board siblings, 2 per-simulation launches around the streamed engine, 3
 * mzx::rt_search_kernel (every simulation in one launch, csrc/mzx_tower_search.inc), 4 the fully connected whole-search
 * kernel; for 3: out[1..6] = {trees per workgroup, row tiles per wave, workgroups, workgroups per CU, LDS bytes, threads per
 * workgroup}; for 2: out[6..7] = trees of the two half-shards (second 0: undivided). */
int mzx_search_route(const mzx_search* s, int32_t out[8]);
/* The same for a search of `num_trees` roots x `num_simulations` on `net` in the default mode, WITHOUT a search handle (no
 * device needed: tests/test_streamed_coverage.py keeps bench.py's workloads inside the GPU-tested launch shapes with it). */
int mzx_net_search_route(const mzx_net* net, int32_t num_trees, int32_t num_simulations, int32_t out[8]);

/* Byte offsets inside the arena (diagnostics): out[0..6] = (unused, 0), trees, hidden states,
 * network workspace, bytes per tree, workspace bytes, total bytes. */
int mzx_search_arena_offsets(const mzx_search* s, int64_t out[8]);

/* Lock-step interface (parity harness, SURVEY.md section 8c'): the tree arithmetic
 * alone, with the network outputs supplied by the caller in binary64.
 *   begin : root expansion from d_root_priors [B][A] (slot order) and d_root_reward (+ io->d_noise)
 *   select: one selection walk per tree -> d_parent/d_action/d_leaf [B]
 *   apply : expand the selected leaf with (value, reward, priors [B][A]) and back-propagate
 *   finish: write io outputs */
int mzx_search_lockstep_begin(mzx_search* s, const mzx_search_io* io, const double* d_root_priors,
                              const double* d_root_reward /* [B], NULL = decoded zero-reward head */,
                              void* d_arena, int64_t arena_bytes, void* stream);
int mzx_search_lockstep_select(mzx_search* s, const mzx_search_io* io, int32_t* d_parent, int32_t* d_action,
                               int32_t* d_leaf, void* d_arena, void* stream);
int mzx_search_lockstep_apply(mzx_search* s, const double* d_value, const double* d_reward,
                              const double* d_priors, void* d_arena, void* stream);
int mzx_search_finish(mzx_search* s, const mzx_search_io* io, void* d_arena, void* stream);

/* Canonical-order dump of the trees (parity tests / diagnose tooling):
 * copies node statistics of every tree into caller arrays sized for
 * num_simulations+1 nodes: visit [B][N] i32, value_sum [B][N] f64, reward [B][N] f64,
 * to_play [B][N] i32, parent [B][N] i32, child [B][N][A] i32, prior [B][N][A] f64,
 * minmax [B][2] f64, n_nodes [B] i32.  Any pointer may be NULL. */
typedef struct mzx_tree_dump {
  int32_t* d_visit; double* d_value_sum; double* d_reward; int32_t* d_to_play; int32_t* d_parent;
  int32_t* d_child; double* d_prior; double* d_minmax; int32_t* d_n_nodes;
} mzx_tree_dump;
int mzx_search_dump(mzx_search* s, const mzx_tree_dump* dump, void* d_arena, void* stream);

/* ------------------------------------------------------------------------- *
 * Continued searches: MCTS.run(..., override_root_with=node) (self_play.py:260-361) on a node that already carries
 * visits and expanded descendants -- a child of the previous move's root (tree reuse) or the same root searched again
 * (anytime budgets).  Semantics: the reference's, bit for bit:
 *   - the new tree holds exactly the subtree under the chosen node, renumbered in creation order (increasing old
 *     canonical index, the new root at 0); the leaf expanded by continued simulation k gets index n_carried + k;
 *     every carried node keeps visit count, value sum, reward, to_play, its children's priors and its hidden state;
 *   - a carried non-root node was expanded over the whole action space: the new root has A children in action order;
 *   - Dirichlet noise (io->d_noise, one value per root child in slot order) is mixed into the children's existing
 *     priors; MinMaxStats starts empty; max_tree_depth counts from the new root; root_predicted_value is NaN;
 *   - io->d_to_play must equal the carried root's to_play.
 *
 * mzx_search_set_capacity: node slots per tree = max_nodes (>= num_simulations + 1) and the pb_c / sqrt tables for
 *   visit counts 0 .. max_nodes - 1 (max_nodes entries each, same definition as in mzx_search_config).  Re-plans the
 *   arena (mzx_search_arena_bytes grows) and forgets what earlier calls left in any arena.  A handle with spare
 *   capacity runs mzx_search_run and mzx_search_run_continued on the same route (mzx_search_route reports it), one that
 *   leaves every node's hidden state in the arena: the fully connected whole-search kernel where its LDS plan holds the
 *   capacity (route 4; it then exports every search), the tower whole-search kernel (3) or the streamed row route (2)
 *   where a fresh search takes them, else the per-operator path (0) -- never the LDS-resident residual kernels (1).
 * mzx_search_advance: tree i -> the subtree under root action d_actions[i] (-1: the old root itself), read from the trees
 *   and hidden states the PRECEDING search call of this handle left in d_src_arena (the arena persists between these
 *   calls, as for mzx_search_dump), written to d_dst_arena (another arena of the same size).  MZX_ERR_INVALID when that
 *   call's route does not leave every node's hidden state in d_src_arena (mzx_search_kernel_name names it), or when the
 *   arenas are the same.  An action that names no expanded child keeps the old root and sets flag 4 in the continued
 *   search's io->d_info[1].
 * mzx_search_load: imports B trees built elsewhere (host arrays in canonical order, parents before children, `max_nodes`
 *   node slots per tree; slot s of the root is root action h_root_actions[i][s], of any other node action s).
 *   Synchronises the stream.  MZX_ERR_INVALID for an inconsistent tree or one that cannot take num_simulations more.
 * mzx_search_run_continued: num_simulations simulations on the trees mzx_search_advance / mzx_search_load put into
 *   d_arena (io->d_observation and io->d_legal_actions are not read).  Reads the carried node counts back (one stream
 *   synchronisation) and fails with MZX_ERR_INVALID when carried nodes + num_simulations + 1 exceed the capacity or when
 *   io->d_to_play differs from a carried root's to_play.  The simulations run where a fresh search of the handle runs
 *   (see mzx_search_set_capacity); mzx_search_kernel_name names the kernel.  On a handle without a network it prepares the roots (noise,
 *   meta words, MinMaxStats) and returns: the caller drives mzx_search_lockstep_select / _apply / mzx_search_finish.
 * ------------------------------------------------------------------------- */
typedef struct mzx_tree_load {
  int32_t max_nodes;               /* node slots per tree in the arrays below */
  const int32_t* h_visit;          /* [B][max_nodes] */
  const double* h_value_sum;       /* [B][max_nodes] */
  const double* h_reward;          /* [B][max_nodes] */
  const int32_t* h_to_play;        /* [B][max_nodes] */
  const int32_t* h_parent;         /* [B][max_nodes], -1 for the root */
  const int32_t* h_child;          /* [B][max_nodes][A] child node of each slot, -1 = not expanded */
  const double* h_prior;           /* [B][max_nodes][A] prior of each slot */
  const float* h_hidden;           /* [B][max_nodes][hidden_size] */
  const int32_t* h_n_nodes;        /* [B] */
  const int32_t* h_root_actions;   /* [B][A] actions of the root's children in slot order, padded with -1 */
} mzx_tree_load;
int mzx_search_set_capacity(mzx_search* s, int32_t max_nodes, const double* h_pb_c_table, const double* h_sqrt_table);
int mzx_search_advance(mzx_search* s, const int32_t* d_actions, void* d_src_arena, void* d_dst_arena, void* stream);
int mzx_search_load(mzx_search* s, const mzx_tree_load* trees, void* d_arena, void* stream);
int mzx_search_run_continued(mzx_search* s, const mzx_search_io* io, void* d_arena, int64_t arena_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Observation pipeline on the device (csrc/mzx_obs.h).
 * mzx_obs_stack replaces GameHistory.get_stacked_observations (self_play.py:513-550) for n_out
 * positions at once, reading a device-resident frame store instead of the Python history lists:
 *   d_frames  [ring][num_games][channels][height][width] fp32,  d_actions [ring][num_games] int32;
 *   the observation / action of game g at history index t live in slot t % ring
 *   (action_history convention of the reference: index 0 holds the leading 0, self_play.py:118).
 * Sample n is (game, index) = (d_game[n], d_time[n]); a NULL d_game means n % num_games, a NULL
 * d_time means time0 + n / num_games.  The caller guarantees 0 <= index and that the frames
 * index - stacked_observations .. index are present (ring >= stacked_observations + 1).
 *   d_out [n_out][channels * (stacked + 1) + stacked][height][width] fp32 = the reference's array
 *   after torch.tensor(...).float() (self_play.py:280-285), bit for bit.
 * mzx_support_to_scalar = models.support_to_scalar (models.py:645-666) of `rows` rows of
 * 2 * support_size + 1 logits -> d_out[rows] (Reanalyse's value decode, replay_buffer.py:361-367).
 * ------------------------------------------------------------------------- */
typedef struct mzx_obs_layout {
  int32_t channels, height, width; /* config.observation_shape */
  int32_t stacked_observations;    /* config.stacked_observations */
  int32_t action_space_size;       /* len(config.action_space) */
  int32_t num_games;               /* games interleaved in the frame store */
  int32_t ring;                    /* history slots per game */
} mzx_obs_layout;
int64_t mzx_obs_stacked_floats(const mzx_obs_layout* layout); /* floats per stacked sample; 0 if invalid */
int mzx_obs_stack(const mzx_obs_layout* layout, const float* d_frames, const int32_t* d_actions,
                  const int32_t* d_game, const int32_t* d_time, int32_t time0, int32_t n_out, float* d_out,
                  void* stream);
int mzx_support_to_scalar(const float* d_logits, int32_t rows, int32_t support_size, float* d_out, void* stream);

/* ------------------------------------------------------------------------- *
 * Per-game random streams (host side, no GPU): replaces the numpy.random calls of one
 * self-play actor -- numpy.random.seed (self_play.py:22), numpy.random.dirichlet (:473), the
 * numpy.random.choice(ties) of the search (:371, drawn on the device from the tape this produces)
 * and SelfPlay.select_action's numpy.random.choice (:229-243) -- for a SHARD of games: stream i is
 * numpy.random.RandomState(seed_i), bit for bit (legacy MT19937 algorithms, csrc/mzx_rng.h).
 * All arrays are host arrays; `idx[k]` selects the stream of the k-th entry.
 * ------------------------------------------------------------------------- */
typedef struct mzx_rng mzx_rng;
int mzx_rng_create(int32_t num_streams, mzx_rng** out);
void mzx_rng_destroy(mzx_rng* r);
/* RandomState(seeds[k]) for streams first .. first + count - 1 (0 <= seed < 2^32). */
int mzx_rng_seed(mzx_rng* r, int32_t first, int32_t count, const uint32_t* seeds);
/* RandomState.get_state() / set_state() of one stream: key[624], pos, has_gauss, cached_gaussian. */
int mzx_rng_get_state(const mzx_rng* r, int32_t i, uint32_t* key, int32_t* pos, int32_t* has_gauss, double* gauss);
int mzx_rng_set_state(mzx_rng* r, int32_t i, const uint32_t* key, int32_t pos, int32_t has_gauss, double gauss);
/* Per-move root draws of `count` games: noise[k][0..n_legal[k]) = dirichlet([alpha] * n_legal[k])
 * (noise == NULL: no exploration noise, nothing drawn), then tape[k][0..tape_words) = the NEXT raw
 * 32-bit words of the stream WITHOUT consuming them (the search consumes some; see mzx_rng_advance). */
int mzx_rng_root_draws(mzx_rng* r, const int32_t* idx, int32_t count, double alpha, const int32_t* n_legal,
                       int32_t action_space_size, double* noise, int32_t tape_words, uint32_t* tape, int32_t n_threads);
/* Consume words[k] raw words of stream idx[k] (what the search reported in info[2]). */
int mzx_rng_advance(mzx_rng* r, const int32_t* idx, int32_t count, const int32_t* words);
/* One RandomState.random_sample() per stream (numpy.random.choice(a, p=...) draws exactly one). */
int mzx_rng_random_sample(mzx_rng* r, const int32_t* idx, int32_t count, double* out);
/* One RandomState.randint(0, n[k]) per stream (numpy.random.choice(list of n) draws exactly that). */
int mzx_rng_randint(mzx_rng* r, const int32_t* idx, int32_t count, const int32_t* n, int32_t* out);
/* numpy.random.choice(actions, p=dist / sum(dist)) of SelfPlay.select_action (self_play.py:236-243) for `count`
 * streams at once: weights [count][row_stride] binary64 (the caller's visit_counts ** (1 / temperature), first
 * n[k] entries of a row are used), out[k] = the chosen POSITION in 0..n[k]-1.  Same arithmetic as the Python
 * statement + numpy's legacy choice: left-to-right sum, division, cumulative sum, division by its last
 * element, one random_sample(), right bisection. */
int mzx_rng_choice_weighted(mzx_rng* r, const int32_t* idx, int32_t count, const double* weights,
                            int32_t row_stride, const int32_t* n, int32_t* out);

/* ------------------------------------------------------------------------- *
 * One self-play MOVE of a shard of games in two host calls (self_play.py:138-181 for B games at once): what an actor
 * does around MCTS.run on the host -- root noise draw (:473), tie-break words, the upload of the move's inputs, the
 * search, the download, the streams' advance, SelfPlay.select_action (:222-245) -- without a Python statement per
 * field in between.  `mzx_move` describes a move: host arrays as the game plugin returns them, ONE pinned host
 * block + ONE device block of the same layout for the inputs and for the outputs (io's device pointers point into
 * d_in / d_out; a field's host copy is at the same offset of h_in / h_out; io.d_observation may point elsewhere when
 * `observation` is NULL = the stacked observations are already on the device; h_in == d_in on a build without a
 * device).  Same arithmetic, same draws in the same order as the calls it replaces (mzx_rng_root_draws,
 * mzx_search_run, mzx_rng_advance, mzx_rng_choice_weighted / mzx_rng_randint), pinned by tests/test_selfplay_move.py.
 * ------------------------------------------------------------------------- */
typedef struct mzx_move {
  int32_t num_games;               /* B */
  int32_t action_space_size;       /* A */
  int32_t tape_words;              /* raw words per game handed to the search for its tie breaks */
  int32_t num_threads;             /* host threads for the per-game draws (persistent pool of the bank) */
  const int32_t* streams;          /* [B] stream of game k in the bank */
  const int32_t* legal_actions;    /* host [B][A], game.legal_actions() padded with -1 (validated: self_play.py:296-301) */
  const int32_t* to_play;          /* host [B] */
  const float* observation;        /* host [B][observation_floats], or NULL (io.d_observation holds them already) */
  int64_t observation_floats;
  double dirichlet_alpha;          /* config.root_dirichlet_alpha */
  int32_t add_exploration_noise;   /* 0: no noise drawn (io.d_noise must be NULL) */
  int32_t flags;                   /* MZX_MOVE_NO_SYNC: return once the download is queued; the caller waits for `stream`
                                      (an event of its own behind the call) before it reads h_out */
  void* h_in;  void* d_in;  int64_t in_bytes;
  void* h_out; void* d_out; int64_t out_bytes;
  mzx_search_io io;
} mzx_move;
#define MZX_MOVE_NO_SYNC 1
/* Draws + upload + mzx_search_run + download + stream synchronisation.  n_legal [B] (out): legal actions per game.
 * On return the outputs are in h_out; the streams have consumed the noise draws but NOT the tie-break words
 * (info[k][2]): a caller that sees the tape-overflow flag (info[k][1] & 1) searches those games again on a longer
 * tape before mzx_selfplay_select. */
int mzx_selfplay_search(mzx_search* s, mzx_rng* r, const mzx_move* m, int32_t* n_legal, void* d_arena,
                        int64_t arena_bytes, void* stream);
/* mzx_rng_advance by words[k], then SelfPlay.select_action for every game: temperature[k] == 0 -> first maximum of
 * the visit counts in legal order; +inf -> randint(0, n_legal[k]); else numpy.random.choice(p = dist / sum(dist)) with
 * dist[j] = pow_table[row(temperature[k])][count_j] -- the caller fills pow_table [num_temperatures][table_stride]
 * with numpy's own integer ** (1 / T) for the distinct finite non-zero temperatures `table_temperatures` (so that
 * the power is the reference's, whatever libm this library was linked with).  visit_counts [B][A] by action (as the
 * search wrote them), action [B] (out): the chosen action. */
int mzx_selfplay_select(mzx_rng* r, const mzx_move* m, const int32_t* n_legal, const int32_t* words,
                        const int32_t* visit_counts, const double* temperature, const double* pow_table,
                        int32_t table_stride, const double* table_temperatures, int32_t num_temperatures,
                        int64_t* action);

/* ------------------------------------------------------------------------- *
 * Self-play draws on the device (opt-in, config.device_draws; csrc/mzx_draws.h holds the definition in full): root noise,
 * tie-break tape and action choice as a pure function of (seed, stream, counter) -- NOT numpy's draws, no mzx_rng involved.
 *   seed: what separates one actor's draws from another's -- mzx.self_play passes the actor's own seed (the one its games
 *     and, on host draws, its bank streams are seeded from), not a value shared by every rank of a job.
 *   Words: Philox4x32-10, key = (seed lo, seed hi ^ 0x53454C46), counter = (stream, counter lo, counter hi,
 *     (purpose << 30) | index); purpose 0 noise, 1 tape, 2 action.  stream k = d_streams[k], or first_stream + k when
 *     d_streams is NULL.  Uniforms: ((w0 << 21) | (w1 >> 11)) * 2^-53, then the same of w2, w3, of consecutive blocks.
 *   Tape: word 4b + j of row k is word j of block index b (a longer tape begins with the shorter one).
 *   Noise: child j < n draws g_j = standard_gamma(dirichlet_alpha) by numpy's legacy algorithm (csrc/mzx_rng.h) from the
 *     uniforms of blocks index (j << 14) | 0, 1, ...; noise_j = g_j / (g_0 + ... + g_{n-1}) (left-to-right binary64 sum),
 *     0.0 for j >= n; 1.0 / n when the sum is 0 or not finite.  n = entries >= 0 of the row of d_legal_actions, or d_n[k]
 *     when d_legal_actions is NULL (continued searches).  d_noise NULL: no noise.
 *   Action: u = first uniform of block (purpose 2, index 0), or d_uniforms[k] (tests).  Temperature 0: first maximum of the
 *     visit counts in legal order; +inf: position min(n - 1, floor(u * n)); else w_j = pow_table[row(T)][count_j] (a count
 *     outside the table weighs 0), inclusive left-to-right prefix P_j, t = u * P_{n-1}: the smallest j with P_j > t, else the
 *     last j with w_j > 0.  d_action[k] = legal[j]; -1 for a row without a legal action or a temperature without a table row.
 * Every pointer is a device pointer.  MZX_ERR_INVALID before any launch for: tape_words < 1, action_space_size > 4096,
 * missing outputs, noise without a row count.  One launch each, a wavefront per game.
 * mzx_selfplay_move_device: mzx_selfplay_search + mzx_selfplay_select with these draws -- legal rows validated on the
 *   host and staged as there (m->streams and the bank are not used), then upload, draws into io.d_noise / io.d_tape
 *   (m->dirichlet_alpha), mzx_search_run, the action choice on io.d_legal_actions / io.d_visit_counts (sel's two row
 *   pointers are ignored; sel NULL: no action choice), download, synchronisation unless MZX_MOVE_NO_SYNC -- all on `stream`.  sel->d_temperature and
 *   the power table must be on the device when the call is made (inside d_in: the call uploads h_in); sel->d_action inside
 *   d_out arrives in h_out.  io.d_noise must be set exactly when m->add_exploration_noise is.
 * ------------------------------------------------------------------------- */
typedef struct mzx_draws {
  uint64_t seed, counter;
  const int32_t* d_streams;        /* [B] nullable */
  int32_t first_stream, num_games, action_space_size, tape_words;
  double dirichlet_alpha;
  const int32_t* d_legal_actions;  /* [B][A] padded with -1, or NULL */
  const int32_t* d_n;              /* [B] children per root, read when d_legal_actions is NULL */
  double* d_noise;                 /* out [B][A], nullable */
  uint32_t* d_tape;                /* out [B][tape_words] */
} mzx_draws;
typedef struct mzx_draws_select {
  const int32_t* d_legal_actions;  /* [B][A] */
  const int32_t* d_visit_counts;   /* [B][A] by action */
  const double* d_temperature;     /* [B] */
  const double* d_pow_table;       /* [num_temperatures][table_stride] */
  const double* d_table_temperatures;
  int32_t table_stride, num_temperatures;
  const double* d_uniforms;        /* [B] nullable */
  int64_t* d_action;               /* out [B] */
} mzx_draws_select;
int mzx_selfplay_draws(const mzx_draws* draws, void* stream);
int mzx_selfplay_select_device(const mzx_draws* draws, const mzx_draws_select* sel, void* stream);
int mzx_selfplay_move_device(mzx_search* s, const mzx_move* m, const mzx_draws* draws, const mzx_draws_select* sel,
                             int32_t* n_legal, void* d_arena, int64_t arena_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * Replay hand-off: the INITIAL prioritised-replay priorities of finished games on the device --
 * ReplayBuffer.save_game, replay_buffer.py:39-51, with compute_target_value (:230-262) -- for G games of T searched
 * positions each (a shard record: games that started and ended together).  Device arrays:
 *   d_root_values [G][T] f64 (root.value(), 0 for an unvisited root), d_rewards [G][T+1] f64 (reward_history, leading 0),
 *   d_to_play [G][T+1] i32, d_discount_pow [td_steps+1] f64 = config.discount ** i computed by the CALLER with the host
 *   language's own pow (the reference's `self.config.discount**i`);
 *   out: d_targets [G][T] f64 (nullable) = compute_target_value, bit for bit (binary64 multiply / add in the reference's
 *   order); d_priorities [G][T] f32 = float32(|root - target| ** per_alpha) (binary64 sqrt for 0.5, identity for 1, device
 *   pow otherwise); d_game_priority [G] f32 (nullable) = numpy.max(priorities).
 * ------------------------------------------------------------------------- */
int mzx_replay_priorities(const double* d_root_values, const double* d_rewards, const int32_t* d_to_play, int32_t num_games,
                          int32_t moves, int32_t td_steps, const double* d_discount_pow, double per_alpha, double* d_targets,
                          float* d_priorities, float* d_game_priority, void* stream);

/* ------------------------------------------------------------------------- *
 * Device-resident replay store (mzx.replay.DeviceGameStore; csrc/mzx_replay.h, csrc/mzx_obs.h): finished games stay in
 * HBM and ReplayBuffer.get_batch (replay_buffer.py:70-138) assembles the trainer's tensors there.  Stateless like the
 * entries above: the caller owns the pool, every pointer is a device pointer.
 * Pool: a game of T searched positions starts at pool row `base` and owns rows base .. base + T, one row per history
 * index (root_values / child_visits / values use the first T of them).  The caller keeps 0 <= base, base + T < rows.
 * The Python store allocates the rows circularly and bounds the buffer in POSITIONS besides replay_buffer_size in games
 * (the one deliberate difference from the reference: the oldest games leave store and stock buffer alike when a new game
 * does not fit); mzx.replay.trainer_tensors(batch, device) binds the outputs to a trainer (trainer.py:140-153).
 * mzx_replay_values: compute_target_value (:230-262) of every position of num_games games (d_base[g], d_len[g] = T) into
 *   pool->d_values, bit for bit (the arithmetic of mzx_replay_priorities; d_discount_pow [td_steps + 1] as there).  One
 *   launch for all the games an ingest or a reanalyse update touched.
 * mzx_replay_positions: the reanalyse sweep's sample list, built on the device.  The positions of num_games games, in the
 *   order given, form one flat sequence of total_positions = sum(d_len) entries; d_first [num_games] i64 is the exclusive
 *   prefix of d_len (both totals computed by the CALLER: O(games) host work per sweep, nothing per position).  Entry e of
 *   the window [first, first + count) becomes d_sample_base / d_sample_len / d_sample_pos [count] -- the three arrays
 *   mzx_replay_batch_io takes; games of T = 0 contribute no entry.  A window that runs past total_positions is refused.
 * mzx_replay_reanalyse_write: Reanalyse's value decode (replay_buffer.py:361-367) of a chunk of such samples, written in
 *   place.  d_value_logits [num_samples][2 * support_size + 1] f32 -> d_out [num_samples] f32, the bits of
 *   mzx_support_to_scalar, and d_root_values[d_sample_base[n] + d_sample_pos[n]] = (double)d_out[n] -- the binary64 the
 *   per-game update uploads.  d_root_values is the pool's root_values column, passed writable (the pool holds it const);
 *   mzx_replay_values afterwards refreshes the n-step targets of the games touched.  One launch.
 * mzx_replay_batch: sample n is position d_pos[n] (0 <= pos <= T) of the game (d_base[n], d_len[n]).
 *   d_observation [n][channels * (stacked + 1) + stacked][height][width] f32 = get_stacked_observations(pos, stacked, A)
 *     after torch.tensor(...).float(), the values of mzx_obs_stack; NULL skips the gather.
 *   targets, make_target (:264-303) for unroll step u = 0 .. num_unroll_steps: d_value / d_reward [n][U + 1] f64,
 *     d_policy [n][U + 1][A] f64, d_action [n][U + 1] i64 -- inside the game the stored entries; at index T value 0, the
 *     stored reward and action, the uniform policy 1 / A; past T zeros, 1 / A and d_absorbing_actions[n][u], the actions the
 *     CALLER drew (numpy.random.choice(action_space), :301; entries of other steps are not read) --, d_gradient_scale
 *     [n][U + 1] i64 = min(U, T + 1 - pos) (:103-111).  d_value == NULL skips the targets (then only the gather runs).
 * ------------------------------------------------------------------------- */
typedef struct mzx_replay_pool {
  const float* d_frames;           /* [rows][channels][height][width] */
  const int32_t* d_actions;        /* [rows] action_history */
  const double* d_rewards;         /* [rows] reward_history */
  const int32_t* d_to_play;        /* [rows] to_play_history */
  const double* d_root_values;     /* [rows] root_values, or the reanalysed values */
  const double* d_child_visits;    /* [rows][action_space_size] */
  double* d_values;                /* [rows] derived: mzx_replay_values */
  int64_t rows;
  int32_t channels, height, width; /* config.observation_shape */
  int32_t action_space_size;       /* len(config.action_space) */
} mzx_replay_pool;
typedef struct mzx_replay_batch_io {
  const int64_t* d_base;           /* [num_samples] */
  const int32_t* d_len;            /* [num_samples] T */
  const int32_t* d_pos;            /* [num_samples] */
  const int32_t* d_absorbing_actions; /* [num_samples][num_unroll_steps + 1] */
  int32_t num_samples, num_unroll_steps, stacked_observations, reserved;
  float* d_observation;
  double* d_value;
  double* d_reward;
  double* d_policy;
  int64_t* d_action;
  int64_t* d_gradient_scale;
} mzx_replay_batch_io;
int mzx_replay_values(const mzx_replay_pool* pool, const int64_t* d_base, const int32_t* d_len, int32_t num_games,
                      int32_t td_steps, const double* d_discount_pow, void* stream);
int mzx_replay_positions(const int64_t* d_base, const int32_t* d_len, const int64_t* d_first, int32_t num_games,
                         int64_t total_positions, int64_t first, int32_t count, int64_t* d_sample_base, int32_t* d_sample_len,
                         int32_t* d_sample_pos, void* stream);
int mzx_replay_reanalyse_write(const float* d_value_logits, int32_t num_samples, int32_t support_size, const int64_t* d_sample_base,
                               const int32_t* d_sample_pos, float* d_out, double* d_root_values, void* stream);
int mzx_replay_batch(const mzx_replay_pool* pool, const mzx_replay_batch_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * Reanalyse with fresh searches (DeviceGameStore.reanalyse_search; csrc/mzx_replay.h): a chunk of the sample list
 * mzx_replay_positions writes is searched under the current weights and its visit distributions and root values become
 * the pool's targets, in place.  Between mzx_replay_positions / mzx_replay_batch (observation only) and mzx_search_run,
 * and between mzx_search_run and mzx_replay_values, the two entries below; one launch each, a wavefront per sample.
 * Sample n is row = d_sample_base[n] + d_sample_pos[n] of the pool.
 * mzx_replay_search_inputs: the mzx_search_io inputs of num_samples roots (A = pool->action_space_size).
 *   d_to_play [n] i32 = pool->d_to_play[row].
 *   d_legal [n][A] i32: d_legal_mask is an optional column u32 [pool->rows][ceil(A / 32)], bit a % 32 of word a / 32 set
 *     when action a is legal at that row (bits past A are ignored).  With it: the set bits in INCREASING action order,
 *     padded with -1.  NULL: the identity 0 .. A-1.  A mask row without a bit yields the identity too and sets bit 0 of
 *     d_input_flags [n] i32 (mzx_search_run needs a non-empty list; mzx_replay_search_write passes such a sample over).
 *     Bit 1: the row lies outside 0 .. pool->rows-1; nothing is read from the pool for it.  0 otherwise.
 *   d_tape [n][tape_words] u32: tie-break words from Philox4x32-10, key (seed lo, seed hi ^ 0x52454153), counter
 *     (first_index + n, sweep_counter lo, sweep_counter hi, block); block b supplies words 4b .. 4b + 3.  first_index is
 *     the index of sample 0 in the sweep's flat sequence; first_index + num_samples <= 2^32.
 *   There is no exploration noise (the sweep passes d_noise = NULL): the targets are a function of (seed, sweep_counter).
 * mzx_replay_search_write: the outputs of that search -- d_visit_counts [n][A] i32, d_root_value [n] f64, d_info [n][4]
 *   i32 -- as targets: d_child_visits[row][a] = (double)visits[a] / (double)sum_a visits[a] (the binary64 quotient of
 *   GameHistory.store_search_statistics, self_play.py:496-511; 0 for an action that is no child; the sum is an integer)
 *   and d_root_values[row] = d_root_value[n].  A sample whose d_info[n][1] is non-zero (tie tape or node overflow), whose
 *   d_input_flags[n] is non-zero or whose visits sum to less than 1 is SKIPPED: both rows keep their contents and
 *   d_skipped[0] (i32, zeroed by the caller before the sweep) grows by one.  d_child_visits / d_root_values are the
 *   pool's columns, passed writable (the pool holds them const); mzx_replay_values afterwards refreshes the n-step targets.
 * ------------------------------------------------------------------------- */
int mzx_replay_search_inputs(const mzx_replay_pool* pool, const uint32_t* d_legal_mask, const int64_t* d_sample_base,
                             const int32_t* d_sample_pos, int32_t num_samples, int32_t tape_words, uint64_t seed,
                             uint64_t sweep_counter, int64_t first_index, int32_t* d_to_play, int32_t* d_legal, uint32_t* d_tape,
                             int32_t* d_input_flags, void* stream);
int mzx_replay_search_write(const int32_t* d_visit_counts, const double* d_root_value, const int32_t* d_info,
                            const int32_t* d_input_flags, int32_t num_samples, int32_t action_space_size,
                            const int64_t* d_sample_base, const int32_t* d_sample_pos, double* d_child_visits,
                            double* d_root_values, int32_t* d_skipped, void* stream);

/* ------------------------------------------------------------------------- *
 * Prioritised sampling and priority feedback for the store above (csrc/mzx_replay.h): the PER priorities live in the pool
 * too, batches are DRAWN on the device and the trainer's new priorities are scattered back there, so get_batch, the loss
 * head and update_priorities are launches on one stream.  Stateless like the entries above: the caller owns every array
 * of mzx_replay_sampler, every pointer is a device pointer, and the argument checks return MZX_ERR_INVALID before
 * anything is launched.
 * State: d_priorities f32 [rows] -- row base + i the priority of position i < T, the padding row base + T 0 --; d_owner
 *   i32 [rows], scratch of the scatter, -1 everywhere between calls; a table of `slots` games, slot = game_id % slots:
 *   d_slot_game i64 (-1: empty), d_slot_base i64, d_slot_len i32 (T), d_slot_priority f32 (the maximum of the game's
 *   priorities: game_priority), d_slot_sum f64 (their sum).  A slot whose rows do not lie inside the pool is never followed.
 *   A priority counts with its float32 value widened to binary64; a non-finite or non-positive one counts as 0.
 *   Workspace: d_tile_prefix f64 [2 * ceil(slots / 256)], d_raw f64 [raw_capacity >= num_samples] (PER only).
 * mzx_replay_sampler_refresh: d_slot_priority (max) and d_slot_sum (binary64 sum) of the n slots listed in d_slots (i32),
 *   recomputed from d_priorities; an empty slot gets 0 / 0.  One launch.
 * mzx_replay_sample: num_samples draws of the reference's two-level distribution (replay_buffer.py:166-202): game by
 *   game_priority, position by priorities; both uniform when per == 0.
 *   Uniforms: Philox4x32-10, key = (seed lo, seed hi), counter = (sample index, call_counter lo, call_counter hi, block).
 *     Block 0 with words w0..w3: u_game = ((w0 << 21) | (w1 >> 11)) * 2^-53, u_pos the same from w2, w3.  d_uniforms f64
 *     [num_samples][2] (nullable) replaces the two.  Blocks 1, 2, ... supply one word per unroll step: absorbing step u takes
 *     index = mulhi(word_u, num_actions) -- no rejection step: bias at most num_actions / 2^32 -- and the action
 *     d_action_space[index] (i32 [num_actions]; NULL: the identity).
 *   Game level: slot weight w_s = (double)slot_priority with per, else 1, for a resident game of T > 0; 0 otherwise.
 *     S = sum w_s, C_s the inclusive prefix in slot order, t = u_game * S: the smallest s with C_s > t.  If rounding leaves
 *     none, the last slot of positive weight.  Position level with per: the same rule over the T priorities, total P =
 *     slot_sum; without: pos = min(T - 1, floor(u_pos * T)).  A level whose total is 0 is drawn uniformly (every live game
 *     with w = 1, S = their number; every position with p = 1, P = T).  No draw leaves the table or its game whatever the
 *     priorities hold.  Sums are binary64 in a fixed association (tiles / chunks of 256): the same bits on every run.
 *   Outputs: d_base / d_len / d_pos / d_absorbing_actions [num_samples][num_unroll_steps + 1] -- the arrays
 *     mzx_replay_batch_io takes; the whole tape row is written: the drawn action at the steps past the end of the game, 0
 *     elsewhere --, d_game_id i64 [num_samples] (-1 with base 0, T 0 when no game is live), and with per d_weight f32
 *     [num_samples]: raw = 1.0 / (((double)total_samples * (w_s / S)) * (p_i / P)), weight = (float)(raw / max raw), all
 *     in binary64 (the reference divides by the maximum in float32: this opt-in path defines its own rounding).  A sample
 *     drawn while no game is live, and every sample when total_samples <= 0, gets the weight 0 (never NaN).
 *   Launches: tile sums, tile prefix, draw (a wavefront per sample), and with per the weight finish.
 * mzx_replay_update_priorities (replay_buffer.py:205-228): sample i writes d_new[i][k] to position d_pos[i] + k for
 *   k < min(steps, T - pos), provided d_slot_game[d_game_id[i] % slots] == d_game_id[i] (otherwise the game has left the
 *   buffer and the sample is passed over).  Where windows overlap the highest sample index wins, as in the reference's
 *   sequential loop: a claim pass (integer atomic max of i into d_owner), a write pass (stores where the claim is its
 *   own, puts -1 back), then slot_priority / slot_sum of the games touched.  Deterministic; three launches.
 * ------------------------------------------------------------------------- */
typedef struct mzx_replay_sampler {
  float* d_priorities;             /* [rows] */
  int32_t* d_owner;                /* [rows] */
  const int64_t* d_slot_game;      /* [slots] */
  const int64_t* d_slot_base;      /* [slots] */
  const int32_t* d_slot_len;       /* [slots] */
  float* d_slot_priority;          /* [slots] */
  double* d_slot_sum;              /* [slots] */
  int64_t rows;
  int32_t slots, reserved;
  double* d_tile_prefix;           /* workspace [2 * ceil(slots / 256)] */
  double* d_raw;                   /* workspace [raw_capacity] */
  int64_t raw_capacity;
} mzx_replay_sampler;
typedef struct mzx_replay_sample_io {
  uint64_t seed, call_counter;
  int64_t total_samples;
  int32_t num_samples, per, num_unroll_steps, num_actions;
  const int32_t* d_action_space;   /* nullable */
  const double* d_uniforms;        /* nullable */
  int64_t* d_base;
  int32_t* d_len;
  int32_t* d_pos;
  int32_t* d_absorbing_actions;
  int64_t* d_game_id;
  float* d_weight;                 /* required with per, ignored without */
} mzx_replay_sample_io;
int mzx_replay_sampler_refresh(const mzx_replay_sampler* sampler, const int32_t* d_slots, int32_t n, void* stream);
int mzx_replay_sample(const mzx_replay_sampler* sampler, const mzx_replay_sample_io* io, void* stream);
int mzx_replay_update_priorities(const mzx_replay_sampler* sampler, const float* d_new, const int64_t* d_game_id,
                                 const int32_t* d_pos, int32_t n, int32_t steps, void* stream);

/* ------------------------------------------------------------------------- *
 * Bulk ingest of finished games into the store above (DeviceGameStore.add_records; csrc/mzx_replay.h): num_games games
 * staged on the device as a shard hands them out -- game-major, ragged, the layout of mzx_actor_take -- become pool rows,
 * sampler priorities and table slots in ONE call, whatever their number and lengths.  Stateless; every pointer is a device
 * pointer.  The pool's columns, the sampler's slot columns (d_slot_game / d_slot_base / d_slot_len) and the mask column
 * are WRITTEN: the structs hold most of them const for their readers, the entry casts that away.
 * Game g has T = d_len[g] searched positions and goes to pool rows d_base[g] .. d_base[g] + T.  Its staged rows start at
 * d_src1[g] in the arrays of T + 1 entries per game and at d_src0[g] in those of T entries: the exclusive prefixes of
 * len + 1 and of len, computed by the CALLER (O(games) host work, as d_first of mzx_replay_positions); total_rows =
 * sum(len + 1).  Staged arrays:
 *   d_observations [total_rows][channels * height * width] f32, d_actions [total_rows] i64, d_rewards [total_rows] f64,
 *   d_to_play [total_rows] i64; d_visits [sum T][A] i32 (visit counts), d_root_values [sum T] f64 (raw search values),
 *   d_legal_mask [sum T][A] u8 (NULL: every action legal), d_priorities [sum T] f32 (NULL: computed here).
 * Pool row base + i, i <= T: the frame copied; actions / to_play narrowed to i32; the reward copied.  For i < T, with
 *   total = the sum of the row's visit counts: root_values = total > 0 ? value : 0.0 and child_visits[a] = legal(a) &&
 *   total > 0 ? (double)visits[a] / (double)total : 0.0 (one binary64 division: Python's int / int).  The padding row i ==
 *   T holds 0.0 and zeros.  d_pool_legal_mask (u32 [mask_rows][ceil(A / 32)], nullable; mask_rows must equal pool->rows):
 *   bit a set iff action a is legal; all-ones words on the padding row and, without d_legal_mask, on every row.
 * sampler (nullable): d_priorities[base + T] = 0; rows i < T get 0 with per == 0, the staged priority with per and
 *   d_priorities, else (float)(|root - value| ** per_alpha) -- the function of mzx_replay_priorities, bit for bit.  Slot
 *   d_game_id[g] % slots takes (game_id, base, T) and its d_slot_priority / d_slot_sum are refreshed.
 * pool->d_values of every ingested game as mzx_replay_values writes it (td_steps, d_discount_pow as there).
 * Launches, on the caller's stream, independent of num_games: the rows (a wavefront per pool row), the n-step values,
 *   and with a sampler the slots.  num_games == 0 succeeds and launches nothing.  MZX_ERR_INVALID, before anything is
 *   launched: a NULL required pointer, num_games < 0 or total_rows < num_games, action_space_size or the frame shape of
 *   the io other than the pool's, sampler->rows or mask_rows other than pool->rows.
 * What the device arrays HOLD is the caller's contract, as in the rest of this section: 0 <= base, base + T < rows, no two
 *   games on one row or in one slot (the Python store checks residency, slots and room before it stages anything).  A
 *   game whose rows would leave the pool is passed over.
 * ------------------------------------------------------------------------- */
typedef struct mzx_replay_ingest_io {
  const int32_t* d_len;            /* [num_games] T */
  const int64_t* d_base;           /* [num_games] destination pool row */
  const int64_t* d_game_id;        /* [num_games] */
  const int64_t* d_src1;           /* [num_games] exclusive prefix of len + 1 */
  const int64_t* d_src0;           /* [num_games] exclusive prefix of len */
  const float* d_observations;
  const int64_t* d_actions;
  const double* d_rewards;
  const int64_t* d_to_play;
  const int32_t* d_visits;
  const double* d_root_values;
  const uint8_t* d_legal_mask;     /* nullable */
  const float* d_priorities;       /* nullable */
  const double* d_discount_pow;    /* [td_steps + 1] */
  double per_alpha;
  int64_t total_rows;              /* sum(len + 1) */
  int32_t num_games, td_steps, per, action_space_size;
  int32_t channels, height, width, reserved;
} mzx_replay_ingest_io;
int mzx_replay_ingest(const mzx_replay_pool* pool, const mzx_replay_sampler* sampler, uint32_t* d_pool_legal_mask,
                      int64_t mask_rows, const mzx_replay_ingest_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * Export of resident games (DeviceGameStore.download_games; csrc/mzx_replay.h): the inverse of the ingest, for reading
 * games back.  num_games games (d_base[g], d_len[g] = T) of the pool are packed on the device, game-major and ragged, in
 * the ingest's staged layout; the caller downloads the packed arrays, one copy per column whatever the number of games.
 * Stateless; every pointer is a device pointer; nothing of the pool is written.
 * Game g's packed rows start at d_dst1[g] in the arrays of T + 1 entries per game and at d_dst0[g] in those of T entries:
 * the exclusive prefixes of len + 1 and of len, computed by the CALLER; total_rows = sum(len + 1).  Packed arrays:
 *   d_observations [total_rows][channels * height * width] f32 (the frames), d_actions [total_rows] i64 and d_to_play
 *   [total_rows] i64 (the pool's i32 widened), d_rewards [total_rows] f64; d_child_visits [sum T][A] f64 -- the pool's
 *   quotients as they lie, NOT visit counts --, d_root_values [sum T] f64 (the pool's column: 0.0 for an unvisited root,
 *   the reanalysed value after a sweep).
 *   Optional: d_legal_mask [sum T][A] u8, 1 where bit a of the row of d_pool_legal_mask (u32 [mask_rows][ceil(A / 32)],
 *   mask_rows must equal pool->rows) is set; d_priorities [sum T] f32, the rows of sampler->d_priorities (only that column
 *   and sampler->rows, which must equal pool->rows, are read).  The padding row base + T contributes to the arrays of T + 1
 *   entries only.
 * One launch on the caller's stream, a wavefront per packed row.  num_games == 0 succeeds and launches nothing.
 * MZX_ERR_INVALID, before anything is launched: a NULL required pointer, num_games < 0 or total_rows < num_games,
 *   d_legal_mask without d_pool_legal_mask or with mask_rows other than pool->rows, d_priorities without a sampler column
 *   of pool->rows rows.
 * A game whose rows would leave the pool (base < 0, T < 0 or base + T >= rows) is passed over: its packed rows keep what
 *   they held.  That d_dst1 / d_dst0 are the prefixes of d_len is the caller's contract, as d_src1 / d_src0 of the ingest.
 * ------------------------------------------------------------------------- */
typedef struct mzx_replay_export_io {
  const int64_t* d_base;           /* [num_games] pool row of the game */
  const int32_t* d_len;            /* [num_games] T */
  const int64_t* d_dst1;           /* [num_games] exclusive prefix of len + 1 */
  const int64_t* d_dst0;           /* [num_games] exclusive prefix of len */
  float* d_observations;
  int64_t* d_actions;
  double* d_rewards;
  int64_t* d_to_play;
  double* d_child_visits;
  double* d_root_values;
  uint8_t* d_legal_mask;           /* nullable */
  float* d_priorities;             /* nullable */
  int64_t total_rows;              /* sum(len + 1) */
  int32_t num_games, reserved;
} mzx_replay_export_io;
int mzx_replay_export(const mzx_replay_pool* pool, const mzx_replay_sampler* sampler, const uint32_t* d_pool_legal_mask,
                      int64_t mask_rows, const mzx_replay_export_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * The loss head of the trainer (mzx.trainer; csrc/mzx_trainer.h): what Trainer.update_weights computes between the
 * network's logits and loss.backward() (trainer.py:161-258).  Stateless; every pointer is a device pointer, fp32.
 * mzx_scalar_to_support = models.scalar_to_support (models.py:669-689) of `rows` scalars -> d_out [rows][2 * support_size
 *   + 1], bit for bit (at most two non-zeros per row; the fused entry below derives the same pair in registers).
 * mzx_trainer_loss, for B = batch samples, steps = num_unroll_steps + 1, W = 2 * support_size + 1, A = num_actions:
 *   in:  d_value_logits / d_reward_logits [steps][B][W], d_policy_logits [steps][B][A] -- STEP-MAJOR, what
 *        torch.stack(list_of_steps, 0) yields --, d_target_value / d_target_reward [B][steps] (scalars),
 *        d_target_policy [B][steps][A] (used as given: rows need not sum to 1), d_gradient_scale [B][steps],
 *        d_weight [B] (the PER weights; NULL when PER is off).
 *   out: d_losses [4] = loss, mean value loss, mean reward loss, mean policy loss (the four numbers update_weights logs):
 *          loss = mean_b(w_b * (value_loss_weight * sum_i vl + sum_{i>=1} rl + sum_i pl)), l = sum_j -t_j * log_softmax(x)_j;
 *        d_priorities [B][steps] = float32(|support_to_scalar(value logits) - target value|) ** per_alpha, the prediction
 *          with the bits of mzx_support_to_scalar;
 *        d_grad_value / d_grad_reward / d_grad_policy, shaped like the logits: d loss / d logit
 *          = (w_b / B) * c_head * g_{b,i} * (softmax(x)_j * sum_j t_j - t_j), c_head = value_loss_weight for the value head,
 *          g_{b,0} = 1, g_{b,i} = 1 / gradient_scale[b][i] (the register_hook lines :225-233; not part of the loss value);
 *          the reward rows of step 0 are written as zeros.  All three NULL: evaluation only.
 *   d_scratch: mzx_trainer_loss_scratch_bytes(batch, steps) bytes, 16-byte aligned.
 *   Two launches (the rows; the batch means in a fixed order), no atomics: the same bits on every run.  MZX_ERR_INVALID
 *   -- before anything is launched -- for batch / steps / num_actions < 1, support_size < 0, a missing required pointer,
 *   gradient pointers given in part, or a short scratch buffer.
 * ------------------------------------------------------------------------- */
typedef struct mzx_trainer_loss_io {
  const float* d_value_logits;
  const float* d_reward_logits;
  const float* d_policy_logits;
  const float* d_target_value;
  const float* d_target_reward;
  const float* d_target_policy;
  const float* d_gradient_scale;
  const float* d_weight;           /* nullable */
  int32_t batch, steps, support_size, num_actions;
  double value_loss_weight, per_alpha;
  float* d_losses;
  float* d_priorities;
  float* d_grad_value;             /* the three gradients: all or none */
  float* d_grad_reward;
  float* d_grad_policy;
  void* d_scratch;
  int64_t scratch_bytes;
} mzx_trainer_loss_io;
int mzx_scalar_to_support(const float* d_x, int32_t rows, int32_t support_size, float* d_out, void* stream);
int64_t mzx_trainer_loss_scratch_bytes(int32_t batch, int32_t steps);
int mzx_trainer_loss(const mzx_trainer_loss_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * One training step of a FULLY CONNECTED network up to and including loss.backward() (csrc/mzx_train_fc.h):
 * Trainer.update_weights (trainer.py:168-262) for MuZeroFullyConnectedNetwork (models.py:80-195) -- the unrolled forward
 * pass, the loss head (the launches of mzx_trainer_loss) and back-propagation through time -- as five launches on one
 * stream, no atomics: the same bits on every run.  B = batch, steps = num_unroll_steps + 1 (steps = 1: no dynamics, the
 * gradients of the dynamics and reward networks are exactly zero); support size and action count are the network's.
 *   in:  d_flat [num_params] the weights in the mzx_net_tensor_info layout (need not be the buffer bound by
 *        mzx_net_set_weights), d_observation [B][input_size], d_action int32 [B][steps] (column 0 unused), and the targets,
 *        gradient scales, PER weights (nullable) and scalars of mzx_trainer_loss_io, with the same meaning.
 *   out: d_grad_flat [num_params] = d loss / d parameter in the layout of d_flat, OVERWRITTEN; d_losses [4] and
 *        d_priorities [B][steps] as mzx_trainer_loss writes them; d_value_logits / d_reward_logits [steps][B][2 S + 1],
 *        d_policy_logits [steps][B][A] (step-major; each optional; the reward rows of step 0 are the constant log-one-hot:
 *        0 at the centre, -inf elsewhere).
 *   min / max of the state normalisation hand their gradient to the selected element, the lowest index on an exact tie.
 *   d_scratch: mzx_train_fc_scratch_bytes(net, batch, steps) bytes, 16-byte aligned (sized for all three logit outputs
 *   absent).
 * mzx_train_fc_supported: 1 when the kernels run this network at this shape, 0 otherwise (residual networks; weights plus
 * per-wave activations beyond the 160 KiB of LDS of a workgroup).  mzx_train_fc_step returns MZX_ERR_INVALID -- before
 * anything is launched -- for batch / steps < 1, a missing required pointer, a short or misaligned scratch buffer or an
 * unsupported network.
 * ------------------------------------------------------------------------- */
typedef struct mzx_train_fc_io {
  const float* d_flat;
  const float* d_observation;
  const int32_t* d_action;
  const float* d_target_value;
  const float* d_target_reward;
  const float* d_target_policy;
  const float* d_gradient_scale;
  const float* d_weight;           /* nullable */
  int32_t batch, steps;
  double value_loss_weight, per_alpha;
  float* d_grad_flat;
  float* d_losses;
  float* d_priorities;
  float* d_value_logits;           /* nullable */
  float* d_reward_logits;          /* nullable */
  float* d_policy_logits;          /* nullable */
  void* d_scratch;
  int64_t scratch_bytes;
} mzx_train_fc_io;
int mzx_train_fc_supported(const mzx_net* net, int32_t batch, int32_t steps);
int64_t mzx_train_fc_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps);
int mzx_train_fc_step(const mzx_net* net, const mzx_train_fc_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * One training step of a RESIDUAL network up to and including loss.backward() (csrc/mzx_train_resnet.h):
 * Trainer.update_weights (trainer.py:168-262) for MuZeroResidualNetwork (models.py:300-623, downsample = False) in
 * TRAINING mode -- BatchNorm normalises with the statistics of the batch, per application of a shared network -- as
 * launches on one stream, no atomics: the same bits on every run.  The convolutions and Linear layers are implicit GEMMs
 * on the FP32 matrix pipes.  The fields of mzx_train_fc_io keep their meaning (d_observation [B][C_in][H][W]) and their
 * place: a layout-identical prefix, asserted in the library (csrc/mzx_train_step.h).  In addition
 *   out: d_stats [mzx_train_resnet_stat_floats(net)]: the running statistics AFTER the step, computed from those in
 *        d_flat: for BatchNorm i in the order of the state_dict, running_mean [C_i] then running_var [C_i], the
 *        BatchNorms behind one another.  The applications of a network fold in forward order (momentum 0.1, the
 *        variance unbiased); a network that is not applied (steps = 1: dynamics) keeps its bits.
 *   d_grad_flat holds exact zeros in the spans of running_mean / running_var.
 *   min / max of the state normalisation hand their gradient to the lowest index on an exact tie.
 * mzx_train_resnet_supported: 0 for a fully connected network, a network with a downsample stem (unless
 * mzx_net_set_train_stem, below, switched its training on), a network without
 * residual blocks, and batch x board < 2 (BatchNorm needs more than one value per channel).
 * mzx_train_resnet_launches: how many launches (kernels and small device-to-device copies) a step makes; 0 if unsupported.
 * mzx_train_resnet_commit_stats: scatter d_stats into the running_mean / running_var spans of d_flat_out (the step after
 * optimizer.step(): whatever the optimizer did to those spans is overwritten); follow it with mzx_net_set_weights.
 * mzx_train_resnet_step returns MZX_ERR_INVALID -- before anything is launched -- for batch / steps < 1, a missing
 * required pointer, a short or misaligned scratch buffer or an unsupported network.
 * ------------------------------------------------------------------------- */
typedef struct mzx_train_resnet_io {
  const float* d_flat;
  const float* d_observation;
  const int32_t* d_action;
  const float* d_target_value;
  const float* d_target_reward;
  const float* d_target_policy;
  const float* d_gradient_scale;
  const float* d_weight;           /* nullable */
  int32_t batch, steps;
  double value_loss_weight, per_alpha;
  float* d_grad_flat;
  float* d_losses;
  float* d_priorities;
  float* d_value_logits;           /* nullable */
  float* d_reward_logits;          /* nullable */
  float* d_policy_logits;          /* nullable */
  void* d_scratch;
  int64_t scratch_bytes;
  float* d_stats;
} mzx_train_resnet_io;
int mzx_train_resnet_supported(const mzx_net* net, int32_t batch, int32_t steps);
int64_t mzx_train_resnet_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps);
int64_t mzx_train_resnet_stat_floats(const mzx_net* net);
int64_t mzx_train_resnet_launches(const mzx_net* net, int32_t batch, int32_t steps);
int mzx_train_resnet_step(const mzx_net* net, const mzx_train_resnet_io* io, void* stream);
int mzx_train_resnet_commit_stats(const mzx_net* net, const float* d_stats, float* d_flat_out, void* stream);

/* ------------------------------------------------------------------------- *
 * Downsample stems (config.downsample = "resnet" / "CNN": games/breakout.py, games/atari.py) are trained natively only
 * on request, per handle.  mzx_net_set_train_stem(net, 1) makes every mzx_train_resnet_* entry plan the stem of the
 * representation network as well: DownSample's two strided 3 x 3 convolutions (no BatchNorm, no bias, no ReLU), its eight
 * BatchNorm residual blocks at C/2 and C channels and its two AvgPool2d(3, 2, 1), or DownsampleCNN's two biased
 * convolutions (+ ReLU), two MaxPool2d(3, 2) and AdaptiveAvgPool2d.  With the switch off (the default) the entries answer
 * as before: supported / scratch_bytes / launches 0, step MZX_ERR_INVALID with "downsample stems ... are not trained
 * natively" in mzx_last_error().  The setter returns MZX_ERR_INVALID for a null handle or a fully connected network; on a
 * residual network without a stem it is accepted and changes nothing.  mzx_net_train_stem reads the switch (0 for null).
 *   Tie rules of the pools (gather form, no atomics: an input element sums the windows that contain or chose it in
 *   increasing window order): AvgPool2d(3, 2, 1) always divides by 9 (count_include_pad); MaxPool2d(3, 2) hands the
 *   gradient to the FIRST maximum of a window in row-major order; window i of AdaptiveAvgPool2d spans
 *   floor(i in / out) .. ceil((i + 1) in / out), overlapping when out > in.
 *   representation_network.module.conv / .bn exist in the state_dict but a stem bypasses them: their spans of d_grad_flat
 *   are exact zeros and their part of d_stats keeps the bits of d_flat (num_batches_tracked must not rise for them).
 *   The input gradient of the layer that reads the observation is never computed.
 * Still refused: networks without residual blocks, batch x board < 2 at ANY BatchNorm (the stem's included), and
 * activations or weight-gradient partials beyond 2^31 elements.
 * ------------------------------------------------------------------------- */
int mzx_net_set_train_stem(mzx_net* net, int on);
int mzx_net_train_stem(const mzx_net* net);

/* ------------------------------------------------------------------------- *
 * The optimizer step over the flat parameter buffer (csrc/mzx_optim.h): torch.optim.Adam (no amsgrad, no maximize) and
 * torch.optim.SGD (dampening 0, no nesterov) as ONE elementwise launch, no atomics: the same bits on every run.
 * Only the LIVE SPANS of the buffer are visited: h_spans [num_spans][2] holds (offset, count) pairs in elements (count
 * 0 is allowed).  Outside them the parameter, the gradient and the state arrays are neither read nor written (a network's
 * running_mean / running_var, the tensors a downsample stem bypasses).  The spans are cut into chunks of at most
 * MZX_OPTIM_CHUNK elements at absolute multiples of that size, one wavefront each: mzx_optim_chunks writes the chunk
 * table (the same pairs) to HOST memory and returns how many chunks there are (h_chunks may be NULL or too short for
 * cap pairs: then nothing is written beyond cap, the count is still returned; MZX_ERR_INVALID for a bad table).  The
 * caller keeps a DEVICE copy of it, d_chunks [num_chunks][2], built once per network.
 *
 * The arithmetic is defined here.  Every operation is IEEE binary32 with gradual underflow, nothing is contracted, `/`
 * and sqrt are correctly rounded.  The caller computes the scalars in binary64 as torch does; the library rounds each to
 * binary32 once.  With g' = g + weight_decay * p (just g when weight_decay == 0):
 *   Adam, step count t >= 1:   m = m + (g' - m) * one_minus_beta1
 *                              v = v * beta2 + (one_minus_beta2 * g') * g'
 *                              den = sqrt(v) / bias_correction2_sqrt + eps
 *                              p = p + (-step_size) * (m / den)
 *     with step_size = lr / (1 - beta1 ** t) and bias_correction2_sqrt = (1 - beta2 ** t) ** 0.5; d_state1 = exp_avg (m),
 *     d_state2 = exp_avg_sq (v).
 *   SGD:  momentum == 0:  p = p + (-lr) * g'  (no state array)
 *         otherwise       buf = g' when first_step (torch: the buffer does not exist yet; it is written, never read),
 *                         else buf = buf * momentum + g';  p = p + (-lr) * buf;  d_state1 = momentum_buffer.
 * 16-byte loads and stores where the alignment of the arrays and of a chunk allows.  Adam moves 28 bytes per element,
 * SGD with momentum 20.
 * mzx_optim_step returns MZX_ERR_INVALID -- before anything is launched -- for a null required pointer, an unknown kind,
 * a span outside [0, n) or two spans that overlap, t < 1, momentum != 0 without d_state1, and a num_chunks that is not
 * what h_spans makes.
 * ------------------------------------------------------------------------- */
#define MZX_OPTIM_CHUNK 1024
#define MZX_OPTIM_ADAM 0
#define MZX_OPTIM_SGD 1
typedef struct mzx_optim_io {
  int32_t kind;                    /* MZX_OPTIM_ADAM / MZX_OPTIM_SGD */
  int32_t first_step;              /* SGD with momentum: the first step */
  int64_t t;                       /* the step count of this step, from 1 */
  float* d_param;                  /* [n] */
  const float* d_grad;             /* [n] */
  float* d_state1;                 /* [n] exp_avg / momentum_buffer (nullable for SGD without momentum) */
  float* d_state2;                 /* [n] exp_avg_sq (Adam) */
  int64_t n;
  const int64_t* h_spans;          /* host [num_spans][2] */
  const int64_t* d_chunks;         /* device [num_chunks][2] (mzx_optim_chunks of h_spans) */
  int32_t num_spans, num_chunks;
  double weight_decay;
  double lr, momentum;                                                             /* SGD */
  double one_minus_beta1, beta2, one_minus_beta2, eps, step_size, bias_correction2_sqrt;      /* Adam */
} mzx_optim_io;
int64_t mzx_optim_chunks(const int64_t* h_spans, int32_t num_spans, int64_t n, int64_t* h_chunks, int64_t cap);
int mzx_optim_step(const mzx_optim_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * Whole training steps queued by ONE call (csrc/mzx_train_chain.h; mzx.trainer.train_steps): num_steps times, on the one
 * stream and in this order,
 *   mzx_replay_sample            call counter first_call + i; seed, total_samples and the slot table as the caller left them
 *   mzx_replay_batch             observation and targets of the drawn samples
 *   a conversion launch          value / reward / policy f64 -> f32, gradient scale i64 -> f32 (round-to-nearest-even),
 *                                action i64 -> i32: what the Python path converts with torch
 *   mzx_train_fc_step or mzx_train_resnet_step   (by the network's kind) reading d_flat, writing d_grad_flat, the four
 *                                losses of step i to d_losses[i][0 .. 3]
 *   the launch of mzx_optim_step   `optim` with t = optim.t + i, first_step only at i == 0, and lr = h_lr[i] (SGD) or
 *                                step_size = h_step_size[i], bias_correction2_sqrt = h_bias_correction2_sqrt[i] (Adam):
 *                                host arrays [num_steps] of binary64 scalars the CALLER computes (the library stays
 *                                stateless); optim.d_param must be d_flat and optim.d_grad d_grad_flat
 *   mzx_train_resnet_commit_stats   for a residual network
 *   mzx_replay_update_priorities    with per
 * and behind the last step mzx_net_set_weights(net, d_flat, ..., d_derived, ...) ONCE: the training kernels read the flat
 * buffer, never the derived one, so a search running beside the chain sees re-folded BatchNorm terms at the granularity
 * of a chain.  The chain calls the functions those entries call; it computes what calling them one by one computes, bit
 * for bit.  No graph capture: plain back-to-back queueing.  Nothing synchronises.
 * d_workspace: mzx_train_chain_scratch_bytes(net, batch, steps) bytes (steps = num_unroll_steps + 1), 256-byte aligned,
 * the caller's, reusable from call to call; its contents mean nothing between calls.  0 bytes: the network's step does
 * not run this shape (mzx_train_chain_supported: 1 / 0).  sampler->raw_capacity >= batch with per.
 * MZX_ERR_INVALID before anything is queued: a null required pointer, num_steps / batch < 1, an unsupported network or
 * shape, a pool whose stacked observation is not the network's input, a short or misaligned workspace, a short derived
 * buffer, and every refusal of mzx_optim_step for each of the steps.
 * ------------------------------------------------------------------------- */
typedef struct mzx_train_chain_io {
  const mzx_replay_pool* pool;
  const mzx_replay_sampler* sampler;
  uint64_t seed, first_call;
  int64_t total_samples;
  int32_t per, num_unroll_steps, stacked_observations, num_actions;
  const int32_t* d_action_space;   /* nullable, as mzx_replay_sample_io */
  int32_t batch, num_steps;
  double value_loss_weight, per_alpha;
  float* d_flat;
  float* d_grad_flat;
  mzx_optim_io optim;
  const double* h_lr;                       /* [num_steps], SGD */
  const double* h_step_size;                /* [num_steps], Adam */
  const double* h_bias_correction2_sqrt;    /* [num_steps], Adam */
  float* d_losses;                 /* [num_steps][4] */
  float* d_derived;
  int64_t derived_floats;
  void* d_workspace;
  int64_t workspace_bytes;
} mzx_train_chain_io;
int mzx_train_chain_supported(const mzx_net* net, int32_t batch, int32_t steps);
int64_t mzx_train_chain_scratch_bytes(const mzx_net* net, int32_t batch, int32_t steps);
int mzx_train_chain(mzx_net* net, const mzx_train_chain_io* io, void* stream);

/* ------------------------------------------------------------------------- *
 * Games that step NATIVELY for a whole shard (host side, no GPU; csrc/mzx_games.h): the plugin surface of
 * games/abstract_game.py:9-105 -- reset / step / legal_actions / to_play -- for num_games games at once, so that a
 * self-play shard need not return to the interpreter per move (mzx_selfplay_rounds below).  kind: "synthetic" (the
 * fixed-shape environment of the metric, mzx/synthetic.py: observation_shape [C,H,W], action_space_size and num_players
 * are read), "tictactoe" / "connect4" / "gomoku" (games/tictactoe.py:125-310, games/connect4.py:125-300,
 * games/gomoku.py:130-300: geometry fixed, the three size arguments are ignored).  seeds [num_games] (nullable = 0).
 * Observations are float32 [num_games][C*H*W] (what torch.tensor(obs).float() makes of the reference game's arrays);
 * mzx_game_info: out[0..7] = C, H, W, actions, players, dtype of the reference game's observation arrays (0 float32,
 * 1 int32, 2 float64), rewards are integers (1 / 0), every action always legal (1 / 0).  legal_actions: int32
 * [num_games][actions], increasing, padded with -1.  mzx_game_reset(games = NULL): every game.
 * ------------------------------------------------------------------------- */
typedef struct mzx_game mzx_game;
int mzx_game_create(const char* kind, int32_t num_games, const uint32_t* seeds, const int32_t* observation_shape,
                    int32_t action_space_size, int32_t num_players, mzx_game** out);
void mzx_game_destroy(mzx_game* g);
int mzx_game_info(const mzx_game* g, int32_t out[8]);
int mzx_game_reset(mzx_game* g, const int32_t* games, int32_t count);
int mzx_game_observe(const mzx_game* g, float* out);
int mzx_game_legal_actions(const mzx_game* g, int32_t* out);
int mzx_game_to_play(const mzx_game* g, int32_t* out);
int mzx_game_step(mzx_game* g, const int64_t* actions, const uint8_t* active /* nullable: games with 0 stay untouched */,
                  double* reward, uint8_t* done);

/* The device-resident twin of a game object (csrc/mzx_games_device.h): the shard's boards, players, keys, step counters
 * and seeds in device memory, played by kernels (one wavefront per game) that call the very rule functions the host
 * object's loops call -- reward, done, observation bits, legal row and side to move equal the host object's for the same
 * actions.  Every array argument is DEVICE memory and every call but create / destroy / download only enqueues on `stream`.
 * create uploads the host object's current state (blocking); download makes the host object that state again and
 * synchronises the stream; the host object must be the kind and size the twin was created from.
 * step: one move of every game; d_actions [num_games] i64; d_active nullable [num_games] u8: a board game with 0 is left
 * untouched (reward 0, not done) -- the synthetic game steps every game, as mzx_game_step does; d_reward [num_games] f64 and
 * d_done [num_games] u8 nullable.  A game that ends is NOT reset here.  An action outside the action space leaves its game
 * untouched (reward 0, not done): the host cannot refuse what it does not see.
 * position: d_obs [num_games][C*H*W] f32, d_legal [num_games][actions] i32 (increasing, padded with -1), d_to_play
 * [num_games] i32, each nullable.  reset: d_games [count] i32 device indices (NULL: every game; entries outside the shard
 * are skipped). */
typedef struct mzx_game_device mzx_game_device;
int mzx_game_device_create(const mzx_game* host, mzx_game_device** out);
void mzx_game_device_destroy(mzx_game_device* d);
int mzx_game_device_step(mzx_game_device* d, const int64_t* d_actions, const uint8_t* d_active, double* d_reward, uint8_t* d_done,
                         void* stream);
int mzx_game_device_position(const mzx_game_device* d, float* d_obs, int32_t* d_legal, int32_t* d_to_play, void* stream);
int mzx_game_device_reset(mzx_game_device* d, const int32_t* d_games, int32_t count, void* stream);
int mzx_game_device_download(const mzx_game_device* d, mzx_game* host, void* stream);

/* ------------------------------------------------------------------------- *
 * The self-play ROUND LOOP of a shard of natively stepped games in one call (self_play.py:110-183 for every slot of the
 * shard + the actor loop :31-52; csrc/mzx_actor.h).  An `mzx_actor` is one SLOT GROUP: its game object, search handle,
 * streams of the bank, staging blocks (`move`: as for mzx_selfplay_search; the host-array fields are the actor's own)
 * and the log of its games in progress.  mzx_selfplay_rounds plays rounds -- one move of every slot: search
 * (mzx_selfplay_search), action draw (mzx_selfplay_select, temperature_threshold gate self_play.py:151-157), Game.step,
 * GameHistory row -- until at least `min_games` games have finished or `max_rounds` (< 0: unbounded) rounds were played;
 * a finished game (done, or max_moves moves) is queued for mzx_actor_take and its slot restarts at once on the same
 * stream.  Two groups take turns on the GPU (one searched while the host consumes the other); nothing is in flight when
 * the call returns.  Temperature: `temperature` applies to the games that START during the call; pow_table as for
 * mzx_selfplay_select (every finite non-zero temperature a running game may carry must have a row).  `retry`: called with
 * the games of a group whose search exhausted its tie-break tape (info flag 1); it must search them again on a longer
 * tape and write visit counts / root value / info into the group's output block (rare; NULL: such a search is an error).
 * In / out: `sequence` numbers finished games in the order they finish (across groups and calls).
 * mzx_actor_take hands out and forgets the finished games of a group, game-major and ragged: game j has length[j] moves;
 * observations / actions / rewards / to_play hold length[j] + 1 entries per game (action_history / reward_history with
 * their leading 0, the final position's observation and side to move), visit_counts / root_values / legal_mask length[j];
 * sizes from mzx_actor_finished (out[0] games, out[1] sum of lengths, out[2] = 1 when a game had a restricted legal set:
 * the legal_mask [sum][A] u8 buffer is then required).  `before_sequence` >= 0 restricts both to the games numbered below it
 * (whole rounds: what the call that returned that `sequence` had finished) -- a caller may take the games of call k from
 * one thread while call k + 1 is running on another (mzx.self_play.SelfPlay.continuous_self_play does).
 * ------------------------------------------------------------------------- */
typedef struct mzx_actor mzx_actor;
typedef struct mzx_actor_config {
  mzx_game* game; mzx_search* search; mzx_rng* bank;
  const int32_t* streams;          /* [num_games] stream of game k in the bank (copied) */
  int32_t first_slot;              /* slot of game 0 in the shard (finished games are reported by shard slot) */
  int32_t max_moves;               /* config.max_moves */
  double temperature;              /* of the games that start with the actor */
  void* d_arena; int64_t arena_bytes;
  mzx_move move;                   /* num_games, action_space_size, tape_words, num_threads, dirichlet_alpha, staging blocks, io */
} mzx_actor_config;
int mzx_actor_create(const mzx_actor_config* config, mzx_actor** out);
void mzx_actor_destroy(mzx_actor* a);
typedef int (*mzx_retry_fn)(void* ctx, int32_t group, int32_t count, const int32_t* games);
typedef struct mzx_rounds {
  double temperature;
  int32_t temperature_threshold;   /* config.temperature_threshold, 0 = none */
  int32_t table_stride;
  const double* pow_table; const double* table_temperatures; int32_t num_temperatures; int32_t reserved;
  int64_t min_games, max_rounds;
  int64_t sequence;                /* in / out */
  mzx_retry_fn retry; void* retry_ctx;
  int64_t rounds, games, searches; /* out: rounds played, games finished, searches run (one per slot and round) */
  double search_seconds;           /* out: host time queueing searches + waiting for them */
  double phase_seconds[6];         /* out: where the host time went -- 0 mzx_selfplay_search (draws, staging, upload, launch,
                                      download queued), 1 waiting for a search's event, 2 the per-move region (action draws, log
                                      row, Game.step, next position), 3 finished games copied out + slots restarted, 4 tape
                                      retries, 5 the rest of the call */
} mzx_rounds;
int mzx_selfplay_rounds(mzx_actor* const* groups, int32_t num_groups, mzx_rounds* io, void* stream);
/* Device draws for a slot group (csrc/mzx_draws.h; before its first round or between calls): from now on the group's moves
 * go through mzx_selfplay_move_device -- seed, counter = first_counter + the number of searches the group has begun since,
 * streams = the group's slots (its `streams` must be consecutive) -- and no stream of the bank is read or advanced.
 * d_temperature [B] f64 inside move.d_in and d_action [B] i64 inside move.d_out: the loop writes every move's temperatures
 * (temperature_threshold gate) into the input block and reads the chosen actions from the output block; the move's
 * io.d_noise / io.d_tape may lie outside the staged blocks (device scratch).  A game whose search raised the tape-overflow
 * flag goes through the retry callback as before (the callback draws the longer tape with mzx_selfplay_draws under the same
 * stream and counter, mzx_actor_draw_counter - 1); its action is then taken by the same function on the host.
 * mzx_actor_draw_counter: the counter of the group's NEXT search (-1 for a null actor). */
int mzx_actor_set_device_draws(mzx_actor* actor, uint64_t seed, uint64_t first_counter, double* d_temperature, int64_t* d_action);
int64_t mzx_actor_draw_counter(const mzx_actor* actor);
/* The counter of the group's next search (a checkpoint's restore); refused while a search is in flight or before
 * mzx_actor_set_device_draws. */
int mzx_actor_set_draw_counter(mzx_actor* actor, uint64_t counter);
/* RESIDENT rounds (csrc/mzx_resident.h; after mzx_actor_set_device_draws, before the group's first round): the group's
 * games (an mzx_game_device made from its game object), its move log and its per-slot bookkeeping live on the device, and
 * mzx_selfplay_rounds queues whole rounds back to back on the group's stream -- draws, search, action choice + vote,
 * commit (log row, step, max_moves cut, finished games recorded and restarted, the next search's inputs and temperatures
 * written straight into the move's input block) -- with no upload, download or wait in between.  The host comes back once
 * per chunk of `chunk_rounds` rounds (fewer at the end of a max_rounds call): one small download (control block and
 * finished list), a gather launch that packs the finished games, one download of those; sequence numbers are assigned on
 * the host in (round, group, slot) order across groups.  Same games, field for field, as the host loop on device draws.
 * Every group of a call must be resident, or none (MZX_ERR_INVALID).  max_rounds is exact.  With min_games the call plays
 * whole chunks and stops at the first chunk end with enough finished games: it may play up to chunk_rounds - 1 rounds more
 * than the host loop would.  io->rounds / searches / games report what was committed; nothing is in flight when the call
 * returns, and the group's host game object holds the device state again (mzx_game_device_download).  A search that
 * exhausts its tie-break tape HALTS the group: nothing commits in that round or behind it, the host searches the round
 * again under the same counter, calls `retry` for the flagged trees (the staging blocks hold the round's inputs and
 * outputs), takes their actions on the host, uploads the patched outputs, commits the round and queues the rest of the
 * chunk again; counters of rounds that did not commit are not consumed.  The device log (max_moves + chunk_rounds + 1 rows
 * per slot and the chunk's finished list) is refused above `max_log_bytes` with a message that states its size.
 * phase_seconds of a resident call: 0 queueing, 1 waiting, 2 unused (0), 3 harvest, 4 repairs, 5 the rest.
 * mzx_actor_resident_stats: out[0] rounds committed, 1 chunks, 2 repair rounds, 3 host synchronisations (stream waits),
 * 4 bytes the rounds calls downloaded, 5 bytes of device log, 6 games harvested, 7 bytes kept on the device in pieces (the
 * device hand-off below; 0 without it). */
int mzx_actor_set_resident(mzx_actor* actor, int32_t chunk_rounds, int64_t max_log_bytes);
int mzx_actor_resident_stats(const mzx_actor* actor, int64_t out[8]);
int mzx_actor_finished(mzx_actor* a, int64_t before_sequence, int64_t out[3]);
int mzx_actor_take(mzx_actor* a, int64_t before_sequence, int32_t* slot, int32_t* length, int64_t* sequence, float* observations, int64_t* actions,
                   double* rewards, int64_t* to_play, int32_t* visit_counts, double* root_values, uint8_t* legal_mask,
                   int32_t* any_illegal);

/* The DEVICE HAND-OFF of a resident group (csrc/mzx_resident.h; opt-in, mzx_actor_set_device_handoff(actor, 1)): the
 * finished games of a chunk are packed on the device and STAY there -- the rounds call downloads nothing of them (out[4] of
 * mzx_actor_resident_stats counts the control blocks and game states only) -- so that mzx_replay_ingest can read them
 * where they lie.  Refused (MZX_ERR_INVALID) for a group that is not resident or that has finished games pending.
 * Harvest: one pack launch per chunk and group, a wavefront per packed row, into a PIECE: a device buffer the actor owns,
 *   holding the packed arrays in the staged layout of mzx_replay_ingest_io -- observations f32 [sum(len + 1)][E], actions /
 *   to_play i64 and rewards f64 [sum(len + 1)], visit counts i32 [sum len][A], root values f64 [sum len], and for a game
 *   whose legal sets vary the legal mask u8 [sum len][A] -- and the columns len i32, src1 / src0 i64 [games] (the
 *   ingest's d_len / d_src1 / d_src0).  Every pack launch has completed when mzx_selfplay_rounds returns.  Sequence
 *   numbers, halts and repairs are those of the default path; the piece's slot / length / sequence stay on the host.
 *   Piece buffers are recycled: a steady-state chunk allocates nothing.  The device log plus the piece buffers the actor
 *   holds are refused above the group's max_log_bytes, with a message that states the sizes.
 * mzx_actor_finished_device: out[0] pieces, out[1] games queued with sequence numbers below before_sequence (-1: all).
 *   A piece belongs to one chunk of one call, so it lies wholly on one side of a call's boundary.
 * mzx_actor_take_device: hands out those pieces, oldest first, while they fit max_pieces / max_games: per piece a row of
 *   MZX_PIECE_INFO_WORDS i64 in piece_info -- token, games, sum len, 1 if a legal mask is present, then the DEVICE addresses
 *   of len, src1, src0, observations, actions, rewards, to_play, visit counts, root values, legal mask (0: none), the
 *   buffer's bytes, 0 -- and per game slot / length / sequence (host arrays, pieces concatenated).  out[0] pieces, out[1]
 *   games handed out.  mzx_actor_finished / mzx_actor_take on such a group return MZX_ERR_INVALID.
 * mzx_actor_download_device: the packed arrays of a taken, unreleased piece into host arrays (NULL: that array is skipped),
 *   one copy per array on `stream`, waited for.  For consumers that need a game on the host after all.
 * mzx_actor_release_device: the piece's buffer may be reused once the work queued on `stream` so far has finished -- the
 *   library records an event there; the host does not wait.  A harvest that finds the event still pending takes another
 *   buffer.  The token is dead afterwards.
 * mzx_actor_destroy waits for the device before it frees the piece buffers, taken ones included. */
#define MZX_PIECE_INFO_WORDS 16
int mzx_actor_set_device_handoff(mzx_actor* actor, int32_t on);
int mzx_actor_finished_device(mzx_actor* actor, int64_t before_sequence, int64_t out[2]);
int mzx_actor_take_device(mzx_actor* actor, int64_t before_sequence, int32_t max_pieces, int64_t max_games, int64_t* piece_info,
                          int32_t* slot, int32_t* length, int64_t* sequence, int64_t out[2]);
int mzx_actor_download_device(mzx_actor* actor, int64_t token, float* observations, int64_t* actions, double* rewards,
                              int64_t* to_play, int32_t* visit_counts, double* root_values, uint8_t* legal_mask, void* stream);
int mzx_actor_release_device(mzx_actor* actor, int64_t token, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MZX_H */
