// mzx_trainer.h -- the loss head of the MuZero trainer on the device: everything between the network's logits and
// loss.backward() in Trainer.update_weights (trainer.py:161-258) -- the categorical targets (models.scalar_to_support,
// models.py:669-689), the three cross-entropy heads of every unroll step (loss_function, trainer.py:286-300), the
// gradient scales of the register_hook lines (:225-233), the PER weights, the batch mean and the PER priorities
// (:197-207, :240-250) -- as ONE launch that also writes the gradient of the loss with respect to every head logit, plus
// a fixed-order finishing launch for the batch means.
//
// Shapes: B samples, `steps` = K + 1 unroll steps, W = 2 * support_size + 1 support bins, A actions.  Logits are
// STEP-MAJOR ([steps][B][width]: what torch.stack(list_of_steps, 0) yields), targets are sample-major ([B][steps]).
//
// The targets are never materialised in the fused kernel: a scalar target has at most two non-zero bins (TargetPair), so
//   l = -(w0 * lsm[i0] + w1 * lsm[i1]),     dl/dx_j = softmax_j * (w0 + w1) - t_j
// with lsm the log-softmax row.  ScalarToSupportOp writes the same pair into dense rows: the reference's fp32 operations
// in the reference's order (bit for bit; the library is compiled with -ffp-contract=off).
//
// Mapping (product build): one wavefront per (sample, step), four per workgroup; the wave runs the value, the reward and
// the policy row one after the other, lanes stride over the bins (consecutive lanes read and write consecutive floats),
// row max / sum of exp / policy dot products are xor-butterflies over the 64 lanes (32, 16, ... 1: every lane ends with
// the same bits, and the same bits on every run -- there is no atomic anywhere).  The rows are re-read from cache for the
// three passes (max, sum, gradient): a row is at most a few KB and belongs to one wave.  The value row is decoded a
// second time in the CANONICAL 16-lane order of mzx_tree.h (element i to lane i % 16, butterfly16_sum) so that the
// prediction behind the priority has the bits of mzx_support_to_scalar for the same logits.
// tests/hostcheck build: the same bodies with one lane (mzx_wave.h), so the sums are taken in increasing bin order -- the two
// builds are each held to the reference, not to each other.
#pragma once
#include "mzx_platform.h"
#include "mzx_tree.h"
#include "mzx_wave.h"

namespace mzx {

// models.scalar_to_support (models.py:669-689) of one scalar: the two scatters as (index, weight) pairs.  fp32, the
// reference's order; 0.001 is rounded to fp32 as torch does for a Python scalar times a float tensor.  At the upper clamp
// the second scatter is masked to (index 0, weight 0); a second scatter that lands on the first one's bin (only possible
// for support_size == 0) overwrites it, as scatter_ does.
struct TargetPair { int i0, i1; float w0, w1; };
MZX_HD inline TargetPair scalar_to_support_pair(float x, int support_size) {
  const float sgn = (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f);
  float t = sqrtf(fabsf(x) + 1.0f) - 1.0f;
  t = sgn * t + 0.001f * x;
  const float S = (float)support_size;
  t = fminf(fmaxf(t, -S), S);
  const float fl = floorf(t);
  float prob = t - fl;
  TargetPair r;
  r.i0 = (int)(fl + S);
  r.w0 = 1.0f - prob;
  const float idx = fl + S + 1.0f;
  const bool masked = 2.0f * S < idx;
  r.i1 = masked ? 0 : (int)idx;
  r.w1 = masked ? 0.0f : prob;
  if (r.i1 == r.i0) r.w0 = r.w1;
  return r;
}

// Dense rows [rows][2 * support_size + 1] of such targets (mzx_scalar_to_support): one element per row.
struct ScalarToSupportOp {
  const float* x;
  float* out;
  int32_t rows, support_size;
  MZX_HD size_t size() const { return (size_t)rows; }
  MZX_HD void operator()(size_t e) const {
    const int W = 2 * support_size + 1;
    float* row = out + e * (size_t)W;
    for (int j = 0; j < W; ++j) row[j] = 0.0f;
    const TargetPair t = scalar_to_support_pair(x[e], support_size);
    row[t.i0] = t.w0;
    row[t.i1] = t.w1;
  }
};

struct alignas(16) TrainerLossRow { float value, reward, policy, pad; };   // the head losses of one (sample, step)

struct TrainerLossParams {
  const float* value_logits;     // [steps][B][W]
  const float* reward_logits;    // [steps][B][W]
  const float* policy_logits;    // [steps][B][A]
  const float* target_value;     // [B][steps]
  const float* target_reward;    // [B][steps]
  const float* target_policy;    // [B][steps][A]
  const float* gradient_scale;   // [B][steps]
  const float* weight;           // [B] nullable (PER off)
  float* priorities;             // [B][steps]
  float* grad_value;             // shaped like the logits; all three null: evaluation only
  float* grad_reward;
  float* grad_policy;
  TrainerLossRow* scratch;       // [B][steps]
  float* losses;                 // [4] total, value mean, reward mean, policy mean
  int32_t batch, steps, support_size, num_actions;
  float value_loss_weight, per_alpha;
};

// float32(|prediction - target|) ** PER_alpha as numpy evaluates it on a float32 array (the exponent rounded to fp32):
// the identity for 1, the IEEE square root for 0.5, otherwise the binary64 pow rounded once.
MZX_HD inline float trainer_priority(float prediction, float target, float per_alpha) {
  const float gap = fabsf(prediction - target);
  if (per_alpha == 1.0f) return gap;
  if (per_alpha == 0.5f) return sqrtf(gap);
  return (float)pow((double)gap, (double)per_alpha);
}

// The factor every logit gradient of (sample b, step i) carries: mean over the batch, PER weight, the head's weight, the
// gradient scale of the register_hook lines (steps >= 1 only) -- in the order autograd applies them.
MZX_HD inline float trainer_grad_factor(const TrainerLossParams& p, int b, int i, float head_weight, bool weighted_head) {
  float c = 1.0f / (float)p.batch;
  if (p.weight) c = c * p.weight[b];
  if (weighted_head) c = c * head_weight;
  if (i > 0) c = c / p.gradient_scale[(size_t)b * p.steps + i];
  return c;
}

constexpr int TRAINER_WAVES = 4;          // wavefronts (rows of the batch) per workgroup of the loss kernel
constexpr int TRAINER_FINISH_BLOCK = 128;

// max and sum of exp(x - max) of a row of n logits, in every lane
MZX_WAVE_FN void wave_row_stats(const float* __restrict__ x, int n, int lane, float& m, float& den) {
  float mx = -MZX_INF;
  WAVE_FOR(j, n) mx = fmaxf(mx, x[j]);
  m = wave_max(mx);
  float acc = 0.f;
  WAVE_FOR(j, n) acc += mzx_expf(x[j] - m);
  den = wave_sum(acc);
}

// One support head (value or reward) of one (sample, step): returns the loss in every lane, writes the gradient row.
MZX_WAVE_FN float wave_support_row(const float* __restrict__ x, float* __restrict__ grad, int W, int support_size, float target,
                                   float c, bool ignored, int lane, float& row_max) {
  if (ignored) {
    if (grad) WAVE_FOR(j, W) grad[j] = 0.0f;
    return 0.0f;
  }
  float m, den;
  wave_row_stats(x, W, lane, m, den);
  row_max = m;
  const float lse = m + logf(den);
  const TargetPair t = scalar_to_support_pair(target, support_size);
  const float l1 = t.i1 == t.i0 ? 0.0f : t.w1 * (x[t.i1] - lse);
  const float loss = -(t.w0 * (x[t.i0] - lse) + l1);
  if (grad) {
    const float tsum = t.i1 == t.i0 ? t.w0 : t.w0 + t.w1;
    WAVE_FOR(j, W) {
      float tj = j == t.i0 ? t.w0 : 0.0f;
      if (j == t.i1 && t.i1 != t.i0) tj = t.w1;
      grad[j] = c * (mzx_div(mzx_expf(x[j] - m), den) * tsum - tj);
    }
  }
  return loss;
}

// support_to_scalar (mzx_tree.h) of a row with 16 lanes at work: lane l holds the partial of canonical lane l % 16
// (elements l % 16, l % 16 + 16, ... in increasing order), the 16 partials are combined by butterfly16_sum -- the
// operations of the serial function in its order, hence its bits.  `m` is the row max (exact in any order).
MZX_WAVE_FN float wave_support_to_scalar(const float* __restrict__ x, int support_size, float m, int lane) {
#ifdef MZX_HOSTCHECK
  return support_to_scalar(x, support_size);
#else
  const int F = 2 * support_size + 1;
  const int j = lane & 15;
  float acc = 0.f;
  for (int i = j; i < F; i += 16) acc += mzx_expf(x[i] - m);
  float part[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) part[k] = lane_value(acc, k);
  const float den = butterfly16_sum(part);
  acc = 0.f;
  for (int i = j; i < F; i += 16) acc += (float)(i - support_size) * mzx_div(mzx_expf(x[i] - m), den);
#pragma unroll
  for (int k = 0; k < 16; ++k) part[k] = lane_value(acc, k);
  return support_inverse_transform(butterfly16_sum(part));
#endif
}

// The three heads of one (sample, step), e sample-major: launch_waves<TRAINER_WAVES>.
struct TrainerLossBody {
  TrainerLossParams p;
  MZX_HD size_t size() const { return (size_t)p.batch * p.steps; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const int b = (int)(e / (size_t)p.steps), i = (int)(e % (size_t)p.steps);
    const int W = 2 * p.support_size + 1, A = p.num_actions;
    const size_t row = (size_t)i * p.batch + b;                                       // step-major logits
    const bool grads = p.grad_value != nullptr;

    const float* xv = p.value_logits + row * W;
    const float tv = p.target_value[e];
    float vmax = 0.f, unused = 0.f;
    const float vl = wave_support_row(xv, grads ? p.grad_value + row * W : nullptr, W, p.support_size, tv,
                                      trainer_grad_factor(p, b, i, p.value_loss_weight, true), false, lane, vmax);
    const float rl = wave_support_row(p.reward_logits + row * W, grads ? p.grad_reward + row * W : nullptr, W, p.support_size,
                                      p.target_reward[e], trainer_grad_factor(p, b, i, 1.0f, false), i == 0, lane, unused);

    const float* xp = p.policy_logits + row * A;
    const float* tp = p.target_policy + e * (size_t)A;
    float m, den;
    wave_row_stats(xp, A, lane, m, den);
    const float lse = m + logf(den);
    float dot = 0.f, tsum = 0.f;
    WAVE_FOR(j, A) {
      const float t = tp[j];
      dot += t * (xp[j] - lse);
      tsum += t;
    }
    dot = wave_sum(dot);
    tsum = wave_sum(tsum);
    if (grads) {
      const float c = trainer_grad_factor(p, b, i, 1.0f, false);
      float* g = p.grad_policy + row * A;
      WAVE_FOR(j, A) g[j] = c * (mzx_div(mzx_expf(xp[j] - m), den) * tsum - tp[j]);
    }

    const float prediction = wave_support_to_scalar(xv, p.support_size, vmax, lane);
    if (lane == 0) {
      p.scratch[e] = TrainerLossRow{vl, rl, -dot, 0.0f};
      p.priorities[e] = trainer_priority(prediction, tv, p.per_alpha);
    }
  }
};

// The batch means: thread t sums samples t, t + 128, ... (per sample the steps in increasing order, as the reference's
// `value_loss += current_value_loss`), then a fixed tree over the 128 partials in LDS.  launch_block<TRAINER_FINISH_BLOCK>.
struct alignas(16) TrainerSums { float total, value, reward, policy; };
struct TrainerFinishBody {
  TrainerLossParams p;
  MZX_WAVE_FN void operator()(int t) const {
    constexpr int THREADS = block_threads(TRAINER_FINISH_BLOCK);
    MZX_BLOCK_SHARED TrainerSums part[THREADS];
    TrainerSums s{0.f, 0.f, 0.f, 0.f};
    for (int b = t; b < p.batch; b += THREADS) {
      float vl = 0.f, rl = 0.f, pl = 0.f;
      for (int i = 0; i < p.steps; ++i) {
        const TrainerLossRow r = p.scratch[(size_t)b * p.steps + i];
        vl += r.value;
        rl += r.reward;
        pl += r.policy;
      }
      float loss = vl * p.value_loss_weight + rl + pl;
      if (p.weight) loss = loss * p.weight[b];
      s.total += loss;
      s.value += vl;
      s.reward += rl;
      s.policy += pl;
    }
    part[t] = s;
    block_sync();
    for (int o = THREADS / 2; o >= 1; o >>= 1) {
      if (t < o) {
        const TrainerSums a = part[t], c = part[t + o];
        part[t] = TrainerSums{a.total + c.total, a.value + c.value, a.reward + c.reward, a.policy + c.policy};
      }
      block_sync();
    }
    for (int k = t; k < 4; k += THREADS) {
      s = part[0];
      const float v = k == 0 ? s.total : (k == 1 ? s.value : (k == 2 ? s.reward : s.policy));
      p.losses[k] = v / (float)p.batch;
    }
  }
};

}  // namespace mzx
