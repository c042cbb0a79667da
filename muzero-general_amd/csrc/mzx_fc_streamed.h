// mzx_fc_streamed.h -- the STREAMED engine for fully connected networks (MuZeroFullyConnectedNetwork, models.py:80-195)
// that the whole-search kernel's plan does not take (fc2_plan, mzx_fused_fc.h: layers up to 64 wide, 16 actions, a support of
// 64, 64 KiB of parameters): a whole inference in ONE launch, every Linear on v_mfma_f32_16x16x4_f32.
//
//   fcs_recurrent_kernel<TM>  gather h_parent through NetIndex, dynamics MLP with the one-hot action, raw state s, reward MLP
//                             on s, min/max scale s -> h, scatter h to the leaf node, policy and value MLPs on h
//   fcs_initial_kernel<TM>    representation MLP on the observation, min/max scale, policy and value MLPs, the constant
//                             reward row (RewardFillOp's)
//
// Work split.  A 256-thread workgroup owns TM rows (trees), TM in {16, 32, 64}: the largest TM whose LDS plan fits and that
// still gives one workgroup per compute unit (fcs_choose_tm; the tuning entry "fcs_tm" forces one).  A row's bits depend
// neither on TM nor on the batch it runs in.
//
// Activations stay in LDS for the whole chain: two ping-pong row buffers [TM][S], S = widest layer rounded up to 16, plus 4
// floats (S / 4 is odd: the 16 rows of a 128-bit read land in 16 different bank quads), and a third buffer [TM][SE] that
// holds s, then h, while the heads run.  The representation network's first layer reads the observation from global memory
// directly, as it reads its weights: no K-slabs through LDS, inputs of any alignment up to FCS_MAX_INPUT.
//
// A Linear is Y = X W^T, issued as D = W-tile . X^T so that a lane ends up with FOUR CONSECUTIVE OUTPUT COLUMNS of one row:
// lane (r = lane & 15, q = lane >> 4) loads W[n0 + r][k0 + 4 q .. + 3] (one 128-bit global load, straight to registers: no
// wave shares a weight element) and X[m0 + r][k0 + 4 q .. + 3] (one ds_read_b128); the pair feeds four MFMAs, MFMA j summing
// k = k0 + 4 q + j over q.  The weights of the next group of 16 k are requested before this group's MFMAs.
//   N >= 64 columns: the four waves divide the column tiles (tile t to wave t & 3), FCS_NB tiles per pass, all TM rows each;
//   N <  64 columns: the four waves divide K (group g to wave g & 3) and own every tile; the partial tiles meet in LDS,
//                    fragment-major, and are summed in the fixed order (w0 + w1) + (w2 + w3) as RtnKsplitGemmBody does.
// No atomics: a second call repeats every bit.  Epilogue in registers, in LinearOp's order: the one-hot action as a gather of
// W[n][E + action[row]], the bias, ELU, then one 128-bit store into the other LDS buffer (columns N .. 16-multiple are
// written as zeros: they are the next layer's zero-fed k) or masked stores to the output tensor.  One barrier per layer (two
// for a split-K one).  Min/max scale: MinMaxScaleOp's arithmetic by a 16-lane row per tree.
//
// Host side: fcs_plan recovers the five MLPs from prog_initial / prog_recurrent and names what it refuses;
// mzx_net_set_fc_engine keeps the plan in the handle (net->fcs; the structs are in mzx_net.h); fcs_run (mzx_fc_streamed.hip)
// launches from it.
#pragma once
#include <algorithm>

#include "mzx_net.h"
#include "mzx_tuning.h"

namespace mzx {

constexpr int FCS_THREADS = 256;
constexpr int FCS_MAX_WIDTH = 1024;            // widest layer served (TM = 16)
constexpr int FCS_MAX_INPUT = 4096;
constexpr int FCS_LDS_BUDGET = 160 * 1024;
constexpr int FCS_KSPLIT_BELOW = 64;           // layers with fewer output columns divide K among the waves

inline bool fcs_take_mlp(const std::vector<OpDesc>& prog, size_t& pos, FcsMlp& m, int in_width, int onehot) {
  m.n = 0;
  int width = in_width + onehot;
  while (pos < prog.size() && prog[pos].kind == OP_LINEAR) {
    const OpDesc& d = prog[pos];
    if (m.n >= MZX_MAX_LAYERS + 1 || d.w_stride != width) return false;
    if (d.use_action != ((m.n == 0 && onehot > 0) ? 1 : 0)) return false;
    FcsLayer& l = m.l[m.n];
    l.w = (int32_t)d.w; l.b = (int32_t)d.b;
    l.K = d.in_features; l.N = d.out_features; l.w_stride = d.w_stride;
    l.elu = d.elu; l.onehot = d.use_action;
    l.vec = (d.w % 4 == 0 && d.w_stride % 4 == 0) ? 1 : 0;
    if (l.K + (l.onehot ? onehot : 0) != width) return false;
    width = d.out_features;
    ++m.n;
    ++pos;
    if (!d.elu) break;
  }
  return m.n > 0 && !m.l[m.n - 1].elu;
}

inline FcsPlan fcs_plan(const mzx_net* net) {
  FcsPlan P;
  if (!net || net->cfg.network != 0) { P.why = "the fully connected streamed engine does not run residual networks"; return P; }
  const int E = (int)net->hidden_size, A = net->cfg.action_space_size, F = net->full_support;
  if (net->input_size > FCS_MAX_INPUT) { P.why = "an observation of more than 4096 values"; return P; }
  if (net->num_params >= (int64_t(1) << 31)) { P.why = "2^31 parameters or more"; return P; }
  P.why = "an operator program that is not representation / scale / policy / value and dynamics / reward / scale / policy / value";
  const std::vector<OpDesc>& pi = net->prog_initial;
  const std::vector<OpDesc>& pr = net->prog_recurrent;
  FcsMlp pol2, val2;
  size_t pos = 0;
  if (!fcs_take_mlp(pi, pos, P.rep, (int)net->input_size, 0)) return P;
  if (pos >= pi.size() || pi[pos].kind != OP_SCALE || pi[pos].len != E || pi[pos].groups_per_sample != 1) return P;
  ++pos;
  if (!fcs_take_mlp(pi, pos, P.pol, E, 0) || !fcs_take_mlp(pi, pos, P.val, E, 0) || pos != pi.size()) return P;
  pos = 0;
  if (!fcs_take_mlp(pr, pos, P.dyn, E, A) || !fcs_take_mlp(pr, pos, P.rew, E, 0)) return P;
  if (pos >= pr.size() || pr[pos].kind != OP_SCALE || pr[pos].len != E || pr[pos].groups_per_sample != 1) return P;
  ++pos;
  if (!fcs_take_mlp(pr, pos, pol2, E, 0) || !fcs_take_mlp(pr, pos, val2, E, 0) || pos != pr.size()) return P;
  if (pol2.n != P.pol.n || val2.n != P.val.n || pol2.l[0].w != P.pol.l[0].w || val2.l[0].w != P.val.l[0].w) return P;
  if (P.rep.l[P.rep.n - 1].N != E || P.dyn.l[P.dyn.n - 1].N != E || P.pol.l[P.pol.n - 1].N != A ||
      P.rew.l[P.rew.n - 1].N != F || P.val.l[P.val.n - 1].N != F) return P;
  P.E = E; P.A = A; P.F = F; P.in_size = (int32_t)net->input_size;
  // LDS-resident rows: the staged state and every layer output except the heads' last (those go to the output tensors)
  auto scan = [&](const FcsMlp& m, bool keeps_last, int which) {
    for (int i = 0; i < m.n; ++i) {
      const FcsLayer& l = m.l[i];
      if (i + 1 < m.n || keeps_last) P.width[which] = std::max(P.width[which], l.N);
      if (l.N < FCS_KSPLIT_BELOW) P.ks_tiles[which] = std::max(P.ks_tiles[which], (l.N + 15) / 16);
    }
  };
  P.width[0] = P.width[1] = E;
  scan(P.rep, true, 0); scan(P.pol, false, 0); scan(P.val, false, 0);
  scan(P.dyn, true, 1); scan(P.rew, false, 1); scan(P.pol, false, 1); scan(P.val, false, 1);
  if (std::max(P.width[0], P.width[1]) > FCS_MAX_WIDTH) { P.why = "a layer wider than 1024"; return P; }
  P.ok = 1;
  P.why = "";
  return P;
}

// LDS row strides and bytes of a chain at TM rows per workgroup
inline int fcs_stride(int width) { return ((width + 15) / 16) * 16 + 4; }
inline int64_t fcs_lds_bytes(const FcsPlan& P, bool recurrent, int TM) {
  const int w = recurrent ? 1 : 0;
  const int64_t part = int64_t(4) * (TM / 16) * P.ks_tiles[w] * 256;      // [wave][row tile][column tile][register][lane]
  return 4 * (int64_t(2) * TM * fcs_stride(P.width[w]) + int64_t(TM) * fcs_stride(P.E) + part);
}

// TM of a launch: the rule fcs_tm_rule of mzx_tuning.h over the tile sizes whose LDS plan fits the budget.  0: nothing fits.
inline int fcs_choose_tm(const FcsPlan& P, bool recurrent, int batch, int forced) {
  bool fits[3];
  for (int i = 0; i < 3; ++i) fits[i] = fcs_lds_bytes(P, recurrent, 16 << i) <= FCS_LDS_BUDGET;
  return fcs_tm_rule(batch, forced, fits);
}

// True when inference `recurrent` of `net` runs on this engine: the handle's switch, which mzx_net_set_fc_engine sets only
// together with the plan it keeps in the handle (net->fcs: the plan is a function of the handle alone).
inline bool fcs_enabled(const mzx_net* net, bool recurrent) {
#ifdef MZX_HOSTCHECK
  (void)net; (void)recurrent;
  return false;      // the serial build keeps running the per-operator program
#else
  (void)recurrent;
  return net && net->fc_engine == MZX_FC_ENGINE_STREAMED && net->fcs.ok;
#endif
}

#ifndef MZX_HOSTCHECK
// Defined in mzx_fc_streamed.hip.  With `ix`, sample b reads hidden-state node ix->in_node[b] of nb.in and writes node
// ix->out_node[b] of nb.hidden.  nb.reward of an initial inference, where given, receives the constant reward row.
int fcs_run(const mzx_net* net, bool recurrent, const NetBuffers& nb, int batch, stream_t stream, const NetIndex* ix);
#endif

}  // namespace mzx
