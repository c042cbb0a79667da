// mzx_train_fc.h -- one training step of a fully connected MuZero network on the device: the unrolled forward pass,
// the loss head and back-propagation through time, i.e. Trainer.update_weights (trainer.py:168-262) up to and including
// loss.backward() for MuZeroFullyConnectedNetwork (models.py:80-195).  The result is d loss / d parameter in the layout
// of the flat weight buffer (mzx_net_tensor_info), overwritten, never accumulated.
//
// Network: five MLPs (models.mlp, :630-642: Linear + ELU per hidden layer, Linear + identity at the end) --
// representation, dynamics, reward, policy, value.  Step 0: s_0 = rep(observation); steps t >= 1: s_t = dyn([h_{t-1},
// one_hot(action_t)]), reward_t = rew(s_t) (the UN-normalised state).  Every step: h_t = (s_t - min s_t) / scale with
// scale = max - min, `+= 1e-5` where scale < 1e-5 (:137-145, :161-168); policy_t = pol(h_t), value_t = val(h_t).  The
// reward logits of step 0 are the constant log-one-hot (0 at the centre bin, -inf elsewhere): no gradient.
//
// Gradient rules that are not plain chain rule:
//   * min / max pass their gradient to the selected element; on an exact tie the LOWEST index takes it (torch picks an
//     index of its own on ties; the golden cases contain none).  The `+= 1e-5` branch has derivative one.
//   * hidden_state.register_hook(grad * 0.5) (trainer.py:178) halves the TOTAL gradient that arrives at h_t, t >= 1:
//     from the policy / value heads of step t and from the dynamics network of step t + 1.  h_0 is not halved, and
//     neither is what the reward head sends into s_t.
//   * 1 / gradient_scale, the PER weights and the batch mean are part of d loss / d logit as mzx_trainer_loss writes it.
//
// Launches of one mzx_train_fc_step (five, whatever the unroll length):
//   1. fc_train_forward_kernel   a wavefront carries ONE sample through all steps, four samples per workgroup; lane j owns
//                                output neuron j (j += 64 for wider layers) of the layer at hand, the layer's input is
//                                read as LDS broadcasts.  The weights are staged once per workgroup in LDS with an odd row
//                                stride (lane j reads row j: conflict-free; the backward pass reads columns: consecutive
//                                lanes, consecutive banks).  Writes the step-major logits and, to scratch, every layer's
//                                output (hidden layers after ELU, the raw states s_t) and the normalised states h_t.
//   2., 3. the launches of mzx_trainer_loss, unchanged: losses, priorities, d loss / d logit.
//   4. fc_train_backward_kernel  the same mapping, steps from the last to the first.  Writes d loss / d pre-activation of
//                                every layer to scratch.  arg-min / arg-max / scale of a state are recomputed from the
//                                stored s_t by the function the forward pass used (same bits), not stored.
//   5. wave_kernel<4, FctWgradBody>  d loss / d W[j][k] = sum over rows (step, sample) of dz[row][j] * x[row][k]: one wavefront
//                                per parameter, lane l sums rows l, l + 64, ... in increasing order, then a xor butterfly
//                                (32, 16, .. 1).  A fixed order, no atomics: the same bits on every run.
// This differs from "per-workgroup partial gradients in LDS + a reduction of partials" in one respect: the partial sums
// live in registers of the wave that owns the parameter, so no gradient image competes with the weights for LDS and no
// cross-wave ordering is needed.  The dot products are 1 to a few hundred wide: vector ALU FMAs, not MFMA.
//
// LDS budget: FCT_LDS_BUDGET = 160 KiB per workgroup (one workgroup per CU) must hold the padded weight image,
// sum over layers of out * (in | 1) + out floats, plus FCT_WAVES * (2 * widest layer + 3 * encoding_size) floats of
// per-wave activations.  cartpole needs 9 KiB, lunarlander 24 KiB, gridworld 17 KiB, simple_grid 8 KiB.
// mzx_train_fc_supported is 0 beyond it, and for residual networks.
//
// Scratch (floats, rows = steps * B, row = step * B + sample; every block 16-byte aligned):
//   loss rows [rows] x 4 | grad value [rows][F] | grad reward [rows][F] | grad policy [rows][A] |
//   value / reward / policy logits (only those the caller did not pass) | h [rows][E] |
//   per layer: out [rows][width] (the heads' last layers are the logits) | per layer: dz [rows][width] (the heads' last
//   layers are the loss head's gradients).
// tests/hostcheck build: the same per-sample functions with one lane (mzx_wave.h), one element per sample, the weights read
// from the flat buffer; the weight gradients are the same wave body, rows in increasing order.
#pragma once
#include <type_traits>
#include <vector>

#include "mzx_launch.h"
#include "mzx_net.h"
#include "mzx_train_step.h"
#include "mzx_trainer.h"

namespace mzx {

constexpr int FCT_WAVES = 4;
constexpr int FCT_LDS_BUDGET = 160 * 1024;
constexpr int FCT_MAX_LAYERS = MZX_MAX_LAYERS + 1;
enum FctMlpId { FCT_REP, FCT_DYN, FCT_REW, FCT_POL, FCT_VAL, FCT_MLPS };

struct FctLayer {
  int32_t in, out;              // `in` counts the one-hot action block of the dynamics network's first layer
  int32_t flat_w, flat_b;       // offsets into the flat weight buffer
  int32_t lds_w, lds_b, ldw;    // the same in the LDS image; ldw = in | 1
  int32_t pad;
  int64_t act, dz;              // scratch offsets of the output rows / the pre-activation gradients; -1: logits / their gradients
};
struct FctMlp { int32_t n, pad; FctLayer l[FCT_MAX_LAYERS]; };
struct FctPlan : TrainHeadPlan {      // A, F and the loss head's scratch offsets
  FctMlp mlp[FCT_MLPS];
  int32_t E, in_size, maxw, lds_weight_floats, wave_floats, num_params;
  int64_t off_h, total_floats;
};
static_assert(std::is_trivially_copyable<FctPlan>::value, "FctPlan travels to the kernels inside FctParams");

struct FctParams {
  FctPlan plan;
  const float* flat;
  const float* obs;
  const int32_t* action;
  float* vlog;
  float* rlog;
  float* plog;
  const float* gv;
  const float* gr;
  const float* gp;
  float* scratch;
  float* grad_flat;
  int32_t B, steps;
};

// Sizes and offsets of a step at (B, steps); false (with the limit named) for what the kernels do not run.
inline bool fct_plan(const mzx_net* net, int32_t B, int32_t steps, bool own_vlog, bool own_rlog, bool own_plog, FctPlan& P,
                     std::string* why = nullptr) {
  auto no = [&](const char* msg) { if (why) *why = msg; return false; };
  if (!net) return no("null network handle");
  if (net->cfg.network != 0) return no("residual networks train through torch (fully connected networks only)");
  if (B < 1 || steps < 1) return no("batch and steps must be positive");
  if (net->num_params >= ((int64_t)1 << 30)) return no("too many parameters");
  const mzx_net_config& c = net->cfg;
  memset(&P, 0, sizeof(P));
  P.E = c.encoding_size; P.A = c.action_space_size; P.F = 2 * c.support_size + 1; P.in_size = (int32_t)net->input_size;
  P.num_params = (int32_t)net->num_params;
  // the Linear operators of the two inference programs, in the order NetBuilder::build_fc emits them
  const int counts[FCT_MLPS] = {c.n_fc_representation_layers + 1, c.n_fc_dynamics_layers + 1, c.n_fc_reward_layers + 1,
                                c.n_fc_policy_layers + 1, c.n_fc_value_layers + 1};
  std::vector<const OpDesc*> lin_i, lin_r;
  for (const OpDesc& d : net->prog_initial) if (d.kind == OP_LINEAR) lin_i.push_back(&d);
  for (const OpDesc& d : net->prog_recurrent) if (d.kind == OP_LINEAR) lin_r.push_back(&d);
  if ((int)lin_i.size() != counts[FCT_REP] + counts[FCT_POL] + counts[FCT_VAL] ||
      (int)lin_r.size() != counts[FCT_DYN] + counts[FCT_REW] + counts[FCT_POL] + counts[FCT_VAL])
    return no("unexpected operator program");
  const OpDesc* const* first[FCT_MLPS] = {lin_i.data(), lin_r.data(), lin_r.data() + counts[FCT_DYN],
                                          lin_i.data() + counts[FCT_REP], lin_i.data() + counts[FCT_REP] + counts[FCT_POL]};
  int64_t lds = 0;
  int maxw = P.in_size;
  if (P.E > maxw) maxw = P.E;
  for (int m = 0; m < FCT_MLPS; ++m) {
    P.mlp[m].n = counts[m];
    for (int l = 0; l < counts[m]; ++l) {
      const OpDesc& d = *first[m][l];
      FctLayer& L = P.mlp[m].l[l];
      L.in = d.w_stride; L.out = d.out_features;
      L.flat_w = (int32_t)d.w; L.flat_b = (int32_t)d.b;
      L.ldw = L.in | 1;
      L.lds_w = (int32_t)lds; lds += (int64_t)L.out * L.ldw;
      L.lds_b = (int32_t)lds; lds += L.out;
      if (L.out > maxw) maxw = L.out;
      if (lds * 4 > FCT_LDS_BUDGET) return no("the weights do not fit the 160 KiB LDS budget of the training kernels");
    }
  }
  P.maxw = maxw;
  P.lds_weight_floats = (int32_t)((lds + 3) & ~(int64_t)3);
  P.wave_floats = (2 * maxw + 3 * P.E + 3) & ~3;
  if (4 * ((int64_t)P.lds_weight_floats + (int64_t)FCT_WAVES * P.wave_floats) > FCT_LDS_BUDGET)
    return no("the weights and per-wave activations do not fit the 160 KiB LDS budget of the training kernels");
  const int64_t rows = (int64_t)B * steps;
  if (rows * maxw >= ((int64_t)1 << 40)) return no("batch x steps too large");
  int64_t o = 0;
  auto take = [&](int64_t floats) { const int64_t at = o; o += (floats + 3) & ~(int64_t)3; return at; };
  train_head_take(P, take, rows, own_vlog, own_rlog, own_plog);
  P.off_h = take(rows * P.E);
  for (int m = 0; m < FCT_MLPS; ++m)
    for (int l = 0; l < P.mlp[m].n; ++l) {
      const bool head_out = (l == P.mlp[m].n - 1) && m >= FCT_REW;
      P.mlp[m].l[l].act = head_out ? -1 : take(rows * P.mlp[m].l[l].out);
      P.mlp[m].l[l].dz = head_out ? -1 : take(rows * P.mlp[m].l[l].out);
    }
  P.total_floats = o;
  return true;
}

// The per-sample functions are wave bodies (mzx_wave.h); what differs between the builds is where the weights are read:
// the padded LDS image of the workgroup, with a barrier after each layer, or the flat buffer.
#ifdef MZX_HOSTCHECK
#define FCT_SYNC() ((void)0)
#define FCT_W(L) ((L).flat_w)
#define FCT_B(L) ((L).flat_b)
#define FCT_LDW(L) ((L).in)
#else
#define FCT_SYNC() __syncthreads()
#define FCT_W(L) ((L).lds_w)
#define FCT_B(L) ((L).lds_b)
#define FCT_LDW(L) ((L).ldw)
#endif

// min, max (first index on ties) and the scale of a state: what representation() / dynamics() normalise with.  Every
// lane walks the E values itself (LDS broadcasts): no cross-lane step, the same bits in both passes.
struct FctNorm { float lo, scale; int imin, imax; };
MZX_WAVE_FN FctNorm fct_norm(const float* s, int E) {
  FctNorm n;
  float lo = s[0], hi = s[0];
  n.imin = 0; n.imax = 0;
  for (int k = 1; k < E; ++k) {
    const float v = s[k];
    if (v < lo) { lo = v; n.imin = k; }
    if (v > hi) { hi = v; n.imax = k; }
  }
  float scale = hi - lo;
  if (scale < 1e-5f) scale += 1e-5f;
  n.lo = lo; n.scale = scale;
  return n;
}

// One MLP forward: input `x` (LDS / local), outputs of layer l to scratch (hidden layers, states) or `last_out` (rows of
// `row`).  `action` >= 0: the one-hot block of the dynamics network's first layer.  Returns where the last layer's
// outputs are (x0 or x1).
MZX_WAVE_FN const float* fct_mlp_forward(const FctParams& p, int m, const float* W, const float* x, float* x0, float* x1, size_t row,
                                    int action, float* last_out, bool valid, int lane) {
  const FctMlp& M = p.plan.mlp[m];
  for (int l = 0; l < M.n; ++l) {
    const FctLayer& L = M.l[l];
    const bool last = l == M.n - 1;
    float* y = (x == x0) ? x1 : x0;
    const int dense = (action >= 0 && l == 0) ? p.plan.E : L.in;
    const int ldw = FCT_LDW(L);
    float* out = (last && last_out) ? last_out : p.scratch + L.act;
    WAVE_FOR(j, L.out) {
      const float* wr = W + FCT_W(L) + (size_t)j * ldw;
      float acc = W[FCT_B(L) + j];
      for (int k = 0; k < dense; ++k) acc = fmaf(wr[k], x[k], acc);
      if (dense != L.in) acc += wr[dense + action];
      if (!last) acc = mzx_elu(acc);
      y[j] = acc;
      if (valid) out[row * L.out + j] = acc;
    }
    FCT_SYNC();
    x = y;
  }
  return x;
}

// Every step of one sample.  buf: 2 * maxw + 3 * E floats of this wave.
MZX_WAVE_FN void fct_forward_sample(const FctParams& p, const float* W, float* buf, int b, bool valid, int lane) {
  const FctPlan& P = p.plan;
  const int E = P.E, F = P.F;
  float* x0 = buf;
  float* x1 = buf + P.maxw;
  float* hn = buf + 2 * P.maxw;
  WAVE_FOR(k, P.in_size) x0[k] = p.obs[(size_t)b * P.in_size + k];
  FCT_SYNC();
  for (int t = 0; t < p.steps; ++t) {
    const size_t row = (size_t)t * p.B + b;
    const float* s;
    if (t == 0) {
      s = fct_mlp_forward(p, FCT_REP, W, x0, x0, x1, row, -1, nullptr, valid, lane);
      WAVE_FOR(j, F) if (valid) p.rlog[row * F + j] = (j == F / 2) ? 0.0f : -(float)MZX_INF;
    } else {
      int a = p.action[(size_t)b * p.steps + t];
      a = a < 0 ? 0 : (a >= P.A ? P.A - 1 : a);
      s = fct_mlp_forward(p, FCT_DYN, W, hn, x0, x1, row, a, nullptr, valid, lane);
    }
    const FctNorm n = fct_norm(s, E);
    FCT_SYNC();          // (every lane has read h_{t-1} and s_t before h_t replaces it)
    WAVE_FOR(k, E) {
      const float h = mzx_div(s[k] - n.lo, n.scale);
      hn[k] = h;
      if (valid) p.scratch[P.off_h + row * E + k] = h;
    }
    FCT_SYNC();
    if (t > 0) fct_mlp_forward(p, FCT_REW, W, s, x0, x1, row, -1, p.rlog, valid, lane);
    fct_mlp_forward(p, FCT_POL, W, hn, x0, x1, row, -1, p.plog, valid, lane);
    fct_mlp_forward(p, FCT_VAL, W, hn, x0, x1, row, -1, p.vlog, valid, lane);
  }
}

// One MLP backward.  `g` (LDS / local, writable): d loss / d output of the last layer.  Writes d loss / d pre-activation
// of every layer that has a scratch block; returns d loss / d input (the first `dense` entries) when `want_dx`.
MZX_WAVE_FN const float* fct_mlp_backward(const FctParams& p, int m, const float* W, float* g, float* x0, float* x1, size_t row,
                                     int dense0, bool want_dx, bool valid, int lane) {
  const FctMlp& M = p.plan.mlp[m];
  for (int l = M.n - 1; l >= 0; --l) {
    const FctLayer& L = M.l[l];
    const bool last = l == M.n - 1;
    if (L.dz >= 0) {
      WAVE_FOR(j, L.out) {
        float d = g[j];
        if (!last) {          // ELU'(z) from a = ELU(z): 1 for a > 0, exp(z) = a + 1 otherwise
          const float a = p.scratch[L.act + row * L.out + j];
          d = d * (a > 0.f ? 1.0f : a + 1.0f);
          g[j] = d;
        }
        if (valid) p.scratch[L.dz + row * L.out + j] = d;
      }
      FCT_SYNC();
    }
    if (l == 0 && !want_dx) break;
    float* dx = (g == x0) ? x1 : x0;
    const int nin = l == 0 ? dense0 : L.in;
    const int ldw = FCT_LDW(L);
    WAVE_FOR(k, nin) {
      const float* wc = W + FCT_W(L) + k;
      float acc = 0.f;
      for (int j = 0; j < L.out; ++j) acc = fmaf(wc[(size_t)j * ldw], g[j], acc);
      dx[k] = acc;
    }
    FCT_SYNC();
    g = dx;
  }
  return g;
}

MZX_WAVE_FN void fct_backward_sample(const FctParams& p, const float* W, float* buf, int b, bool valid, int lane) {
  const FctPlan& P = p.plan;
  const int E = P.E, F = P.F, A = P.A;
  float* x0 = buf;
  float* x1 = buf + P.maxw;
  float* gh = buf + 2 * P.maxw;      // d loss / d h_t, what has arrived so far
  float* gs = gh + E;                // d loss / d s_t
  float* st = gs + E;                // s_t
  WAVE_FOR(k, E) gh[k] = 0.0f;
  FCT_SYNC();
  for (int t = p.steps - 1; t >= 0; --t) {
    const size_t row = (size_t)t * p.B + b;
    const float* state_rows = p.scratch + (t == 0 ? P.mlp[FCT_REP].l[P.mlp[FCT_REP].n - 1].act : P.mlp[FCT_DYN].l[P.mlp[FCT_DYN].n - 1].act);
    WAVE_FOR(k, E) st[k] = state_rows[row * E + k];
    // the two heads that read h_t
    WAVE_FOR(j, A) x0[j] = p.gp[row * A + j];
    FCT_SYNC();
    const float* dp = fct_mlp_backward(p, FCT_POL, W, x0, x0, x1, row, E, true, valid, lane);
    WAVE_FOR(k, E) gh[k] += dp[k];
    FCT_SYNC();
    WAVE_FOR(j, F) x0[j] = p.gv[row * F + j];
    FCT_SYNC();
    const float* dv = fct_mlp_backward(p, FCT_VAL, W, x0, x0, x1, row, E, true, valid, lane);
    WAVE_FOR(k, E) gh[k] = t > 0 ? (gh[k] + dv[k]) * 0.5f : gh[k] + dv[k];
    FCT_SYNC();
    // h = (s - min) / scale, scale = max - min (+ 1e-5): q = g / scale goes to s, -sum q to min, -sum q h to scale
    const FctNorm n = fct_norm(st, E);
    float sum_q = 0.f, sum_qh = 0.f;
    for (int k = 0; k < E; ++k) {
      const float q = mzx_div(gh[k], n.scale);
      sum_q += q;
      sum_qh += q * mzx_div(st[k] - n.lo, n.scale);
    }
    const float dscale = -sum_qh;
    WAVE_FOR(k, E) {
      float d = mzx_div(gh[k], n.scale);
      if (k == n.imin) d += -sum_q - dscale;
      if (k == n.imax) d += dscale;
      gs[k] = d;
    }
    FCT_SYNC();
    if (t > 0) {      // the reward head reads s_t
      WAVE_FOR(j, F) x0[j] = p.gr[row * F + j];
      FCT_SYNC();
      const float* dr = fct_mlp_backward(p, FCT_REW, W, x0, x0, x1, row, E, true, valid, lane);
      WAVE_FOR(k, E) gs[k] += dr[k];
      FCT_SYNC();
      const float* dh = fct_mlp_backward(p, FCT_DYN, W, gs, x0, x1, row, E, true, valid, lane);
      WAVE_FOR(k, E) gh[k] = dh[k];
      FCT_SYNC();
    } else {
      fct_mlp_backward(p, FCT_REP, W, gs, x0, x1, row, 0, false, valid, lane);
    }
  }
}

// d loss / d parameter e: which layer it belongs to, its rows, and the two factors of a row.
struct FctElement {
  const float* dz; int dz_stride;       // dz[row * dz_stride]
  const float* x; int x_stride;         // x[(row - x_shift) * x_stride]; nullptr: bias (1) or the one-hot block
  int64_t x_shift;
  int onehot;                            // >= 0: x = (action of the row == onehot)
  int64_t r0, r1;
};
MZX_HD inline bool fct_element(const FctParams& p, int e, FctElement& out) {
  const FctPlan& P = p.plan;
  const int64_t rows = (int64_t)p.B * p.steps;
  for (int m = 0; m < FCT_MLPS; ++m) {
    const FctMlp& M = P.mlp[m];
    for (int l = 0; l < M.n; ++l) {
      const FctLayer& L = M.l[l];
      const bool is_w = e >= L.flat_w && e < L.flat_w + L.in * L.out;
      const bool is_b = e >= L.flat_b && e < L.flat_b + L.out;
      if (!is_w && !is_b) continue;
      const int j = is_w ? (e - L.flat_w) / L.in : e - L.flat_b;
      const int k = is_w ? (e - L.flat_w) % L.in : 0;
      const bool last = l == M.n - 1;
      const float* dz = p.scratch + L.dz;
      if (last && m == FCT_REW) dz = p.gr;
      if (last && m == FCT_POL) dz = p.gp;
      if (last && m == FCT_VAL) dz = p.gv;
      out.dz = dz + j; out.dz_stride = L.out;
      out.r0 = (m == FCT_DYN || m == FCT_REW) ? p.B : 0;
      out.r1 = m == FCT_REP ? p.B : rows;
      out.x = nullptr; out.x_stride = 0; out.x_shift = 0; out.onehot = -1;
      if (is_w) {
        out.x_stride = L.in;
        if (l > 0) out.x = p.scratch + M.l[l - 1].act + k;
        else if (m == FCT_REP) out.x = p.obs + k;
        else if (m == FCT_REW) out.x = p.scratch + P.mlp[FCT_DYN].l[P.mlp[FCT_DYN].n - 1].act + k;
        else if (m == FCT_DYN) {
          out.x_stride = P.E;
          if (k < P.E) { out.x = p.scratch + P.off_h + k; out.x_shift = p.B; }      // h of the step before
          else out.onehot = k - P.E;
        } else { out.x = p.scratch + P.off_h + k; out.x_stride = P.E; }
      }
      return true;
    }
  }
  return false;
}
MZX_HD inline float fct_element_term(const FctParams& p, const FctElement& el, int64_t r) {
  const float d = el.dz[r * el.dz_stride];
  if (el.x) return d * el.x[(r - el.x_shift) * el.x_stride];
  if (el.onehot >= 0) {
    const int64_t t = r / p.B, b = r % p.B;
    int a = p.action[b * p.steps + t];
    a = a < 0 ? 0 : (a >= p.plan.A ? p.plan.A - 1 : a);
    return a == el.onehot ? d : 0.0f;
  }
  return d;
}

// d loss / d parameter e: launch_waves<FCT_WAVES>, a wavefront per parameter, rows in increasing order per lane
struct FctWgradBody {
  FctParams p;
  MZX_HD size_t size() const { return (size_t)p.plan.num_params; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    FctElement el;
    float acc = 0.f;
    if (fct_element(p, (int)e, el))
      for (int64_t r = el.r0 + lane; r < el.r1; r += WAVE_LANES) acc += fct_element_term(p, el, r);
    acc = wave_sum(acc);
    if (lane == 0) p.grad_flat[e] = acc;
  }
};

// The forward (phase 0) / backward (phase 1) pass; the weight gradients follow the backward pass as a launch of their own.
#ifdef MZX_HOSTCHECK

struct FctForwardOp {
  FctParams p;
  size_t size() const { return (size_t)p.B; }
  void operator()(size_t b) const {
    std::vector<float> buf((size_t)p.plan.wave_floats);
    fct_forward_sample(p, p.flat, buf.data(), (int)b, true, 0);
  }
};
struct FctBackwardOp {
  FctParams p;
  size_t size() const { return (size_t)p.B; }
  void operator()(size_t b) const {
    std::vector<float> buf((size_t)p.plan.wave_floats);
    fct_backward_sample(p, p.flat, buf.data(), (int)b, true, 0);
  }
};

inline int fct_launch(const FctParams& p, int phase, stream_t stream) {
  if (phase == 0) { FctForwardOp op; op.p = p; return launch<64>(op, stream); }
  FctBackwardOp bw; bw.p = p;
  return launch<64>(bw, stream);
}

#else

// The padded weight image of the whole network: every thread of the workgroup copies its share.
__device__ __forceinline__ void fct_stage_weights(const FctParams& p, float* lds) {
  for (int m = 0; m < FCT_MLPS; ++m)
    for (int l = 0; l < p.plan.mlp[m].n; ++l) {
      const FctLayer& L = p.plan.mlp[m].l[l];
      const int n = L.in * L.out;
      for (int e = threadIdx.x; e < n; e += 64 * FCT_WAVES) lds[L.lds_w + (e / L.in) * L.ldw + e % L.in] = p.flat[L.flat_w + e];
      for (int e = threadIdx.x; e < L.out; e += 64 * FCT_WAVES) lds[L.lds_b + e] = p.flat[L.flat_b + e];
    }
  __syncthreads();
}

// Every wave of a workgroup runs the same sequence of barriers: a wave past the end of the batch computes sample B - 1
// again and stores nothing.
__global__ void __launch_bounds__(64 * FCT_WAVES) fc_train_forward_kernel(const FctParams p) {
  extern __shared__ float4 fct_lds4[];
  float* lds = (float*)fct_lds4;
  fct_stage_weights(p, lds);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * FCT_WAVES + wave;
  fct_forward_sample(p, lds, lds + p.plan.lds_weight_floats + wave * p.plan.wave_floats, b < p.B ? b : p.B - 1, b < p.B, lane);
}

__global__ void __launch_bounds__(64 * FCT_WAVES) fc_train_backward_kernel(const FctParams p) {
  extern __shared__ float4 fct_lds4[];
  float* lds = (float*)fct_lds4;
  fct_stage_weights(p, lds);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x * FCT_WAVES + wave;
  fct_backward_sample(p, lds, lds + p.plan.lds_weight_floats + wave * p.plan.wave_floats, b < p.B ? b : p.B - 1, b < p.B, lane);
}

inline int fct_launch(const FctParams& p, int phase, stream_t stream) {
  static std::atomic<uint64_t> fw_done{0}, bw_done{0};
  const int lds_bytes = 4 * (p.plan.lds_weight_floats + FCT_WAVES * p.plan.wave_floats);
  const unsigned grid = (unsigned)((p.B + FCT_WAVES - 1) / FCT_WAVES);
  if (phase == 0) {
    if (const int rc = allow_large_lds((const void*)fc_train_forward_kernel, FCT_LDS_BUDGET, fw_done)) return rc;
    hipLaunchKernelGGL(fc_train_forward_kernel, dim3(grid), dim3(64 * FCT_WAVES), lds_bytes, stream, p);
    return (int)hipGetLastError();
  }
  if (const int rc = allow_large_lds((const void*)fc_train_backward_kernel, FCT_LDS_BUDGET, bw_done)) return rc;
  hipLaunchKernelGGL(fc_train_backward_kernel, dim3(grid), dim3(64 * FCT_WAVES), lds_bytes, stream, p);
  return (int)hipGetLastError();
}

#endif  // MZX_HOSTCHECK

}  // namespace mzx
