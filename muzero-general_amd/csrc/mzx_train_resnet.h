// mzx_train_resnet.h -- one training step of a residual MuZero network on the device: the unrolled forward pass in
// TRAINING mode (BatchNorm on batch statistics), the loss head and back-propagation through time, i.e.
// Trainer.update_weights (trainer.py:168-262) up to and including loss.backward() for MuZeroResidualNetwork
// (models.py:300-623, downsample = False).  Outputs: d loss / d parameter in the layout of the flat weight buffer
// (overwritten; exact zeros in the spans of running_mean / running_var), the BatchNorm running statistics after the step
// (packed, see below), and the logits, losses and priorities exactly as mzx_train_fc_step returns them.
//
// Networks and applications.  The operator programs of the handle (prog_initial / prog_recurrent) are cut into six
// chains of layers: the representation tower (applied once), the dynamics tower (steps - 1 times), the prediction tower
// (steps times) and the reward / value / policy heads (conv1x1 -> flatten -> Linear [+ ELU] ...).  A layer keeps, for
// EVERY application a, its convolution output z (BatchNorm layers), its output y and d loss / d z ("dz") in scratch as
// [application][sample][channel][board]: the applications of a layer lie behind one another with a constant stride, so
//   * everything that does not depend on the step before -- the prediction tower, the three heads, every weight
//     gradient -- runs ONCE over steps x B samples with per-application BatchNorm statistics, and
//   * only the dynamics tower (and the state normalisation between its applications) is launched step by step.
//
// One convolution geometry.  Every layer with weights is a convolution: a ksize x ksize kernel (taps = ksize^2) at `stride`
// with `pad` zeros around the input board Hin x Win, giving the output board H x W.  The plan fills these fields for every
// layer -- conv3x3 on one board: 3, 1, 1; conv1x1: 1, 1, 0; a Linear layer: 1, 1, 0 on a 1 x 1 board; the strided and padded
// convolutions of a stem: their own -- and one set of operand functions (rtn_pos, rtn_im2col, rtn_a / rtn_b / rtn_store<MODE>)
// serves them all, without a special case: the divisors (taps, kernel size, stride) are wave-uniform and known to the host,
// which prepares a multiplier and a shift for each (RtnDiv), so a division costs every geometry one v_mul_hi_u32.
//
// The three GEMMs (RtnGemmBody<MODE, WIDE>, a wavefront per 16 x 16 output tile on v_mfma_f32_16x16x4_f32, operands gathered
// on the fly, ragged tiles masked):
//   forward          M = output positions (sample, y, x)   N = Cout        K = Cin x taps    A = im2col(x), B = W^T
//   input gradient   M = INPUT positions                   N = Cin (real)  K = Cout x taps   A = dz at the outputs a tap reaches, B = W
//   weight gradient  M = Cout                              N = Cin x taps  K = output positions   A = dz^T, B = im2col(x)
// The action plane of the dynamics input is one more (virtual) input channel, ci >= creal, zero in the padding like the
// others; the input gradient covers the real channels only.  The epilogues, each nullable or a flag: bias, ELU or ReLU
// (forward); ELU', an added gradient, its ReLU mask (input gradient).
// The weight gradient cuts its reduction (all applications, all samples, the whole board) into chunks of RTN_KCHUNK
// positions; chunk partials go to scratch and RtnWgradFinishOp sums them in increasing chunk order.  No atomics anywhere:
// a second call reproduces every bit.  MFMA operand layout: lane l feeds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15],
// and holds D[4 (l >> 4) + r][l & 15] in accumulator register r.
//
// One precision switch, bool WIDE: a template parameter of the step (RtnRun<WIDE>) and so of every GEMM and BatchNorm
// kernel of it; true for a network with a downsample stem, false for every other.  WIDE = false: a GEMM keeps four binary32
// accumulator chains over K, and BatchNorm keeps its batch statistics and backward sums, and normalises, in binary32.
// WIDE = true: every MFMA starts from zero and is added to binary64 accumulators, and the statistics type S of RtnBn<S> is
// double.  Only the accumulate step and the join of the GEMM differ, and the BatchNorm kernels are written once in S.
//
// BatchNorm in training mode, per application: RtnBnStatBody (a wavefront per (application, channel): mean, biased
// variance in two passes), RtnBnFoldOp (running statistics, applications in forward order, unbiased variance),
// RtnBnApplyOp (normalise + residual + ReLU).  Every sum of these kernels, the bias gradients and the chunk sums of the
// weight gradients is taken in binary64 and rounded once: the reductions are memory-bound, and the reference's CPU
// BatchNorm accumulates in binary64 as well.  Backward: RtnBnSumsBody (sum g, sum g x^ per (application, channel), g
// masked by the ReLU), RtnBnDzOp (dz = gamma / sigma (g - mean g - x^ mean(g x^))), and after the last application
// RtnBnParamGradOp (d gamma, d beta summed over the applications in increasing order).
//
// State normalisation per (sample, channel) over the board (RtnScaleFwdBody / RtnScaleBwdBody): min and max hand their
// gradient to ONE element, the lowest index on a tie (post-ReLU states tie at 0.0 all the time); `scale += 1e-5` where
// scale < 1e-5 has derivative one.  The 0.5 hook of trainer.py:178 multiplies the TOTAL gradient that reaches the
// normalised state of step t >= 1 (prediction tower of step t + dynamics tower of step t + 1); what the reward head
// sends into the raw state is added after it.
//
// Running statistics output ("stats"): for BatchNorm i of net->bns, 2 C_i floats -- running_mean then running_var --
// at offset sum_{j < i} 2 C_j: mzx_train_resnet_stat_floats(net) floats.  It starts as a copy of the statistics in
// d_flat and every application folds into it; BatchNorms of networks that are not applied (steps = 1: dynamics) keep
// their bits.  mzx_train_resnet_commit_stats scatters it into a flat buffer.
//
// Scratch (floats, every block 16-byte aligned): loss rows | grad value / reward / policy | logits the caller did not
// pass | h [steps][B][C][HW] | d loss / d h from the prediction tower [steps][B][C][HW] | d loss / d s from the reward
// head [steps - 1][B][C][HW] | d loss / d h from the next dynamics application [B][C][HW] | two gradient buffers
// [steps][B][C][HW] | weight-gradient chunk partials | per layer: z, y, dz [applications][B][Cout][HW], BatchNorm
// mean / 1/sigma / variance [applications][3][C] and the two backward sums [applications][2][C] (in S: doubles when WIDE).
//
// Downsample stems (cfg.downsample; planned only when mzx_net_set_train_stem switched the handle on, refused by name
// otherwise): the head of prog_initial -- DownSample's two strided 3 x 3 convolutions without BatchNorm, its eight blocks
// at C / 2 and C channels and its two AvgPool2d(3, 2, 1), or DownsampleCNN's two biased convolutions (+ ReLU), its two
// MaxPool2d(3, 2) and its AdaptiveAvgPool2d -- joins the representation chain.  Layers carry their own channel count and
// boards (the one geometry above), the pools are element kernels in gather form (below),
// the layer that reads the observation gets no input gradient, and representation_network.module.conv / .bn, which the
// stem bypasses, keep zero gradients and their statistics (RtnPlan::idle).
//
// tests/hostcheck build: the same operator list; a GEMM tile is three plain loops over the same operand functions, in the
// order of k that WIDE selects (one fmaf chain, or four 4-term chains per 16 values of k added to a double).
#pragma once
#include <string>
#include <type_traits>
#include <vector>

#include "mzx_launch.h"
#include "mzx_net.h"
#include "mzx_train_step.h"
#include "mzx_trainer.h"
#include "mzx_wave.h"

namespace mzx {

constexpr int RTN_WAVES = 4;
constexpr int RTN_KCHUNK = 512;       // positions per weight-gradient chunk: a constant, so the sums do not depend on the device
constexpr float RTN_BN_EPS = 1e-5f;
constexpr double RTN_BN_MOMENTUM = 0.1;
enum RtnMode { RTN_FWD, RTN_DGRAD, RTN_WGRAD };

// ------------------------------------------------------------------------------------------------ the GEMMs

// n / d for 0 <= n < 2^31 by one multiplication, for a divisor the host knows (Granlund & Montgomery 1994, figure 4.1:
// mul = floor(2^32 (2^shift - d) / d) + 1 with shift = ceil(log2 d); n < 2^31 keeps the sum below from overflowing).  The
// divisors of the geometry are wave-uniform but not compile-time constants, and the instruction sequence of a general
// integer division per gathered element made the step 8 - 14 % slower (profiles/resnet_train_refactor_ab.txt).
struct RtnDiv { uint32_t mul, shift; };
inline RtnDiv rtn_div_by(int d) {
  RtnDiv r;
  r.shift = 0;
  while (((int64_t)1 << r.shift) < d) ++r.shift;
  r.mul = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << r.shift) - (uint64_t)d)) / (uint64_t)d + 1);
  return r;
}
MZX_HD inline int rtn_div(int n, const RtnDiv& d) {
  return (int)(((uint32_t)(((uint64_t)(uint32_t)n * d.mul) >> 32) + (uint32_t)n) >> d.shift);
}

struct RtnGemm {
  const float* x;          // FWD / WGRAD: the layer's input [nb][creal][Hin][Win]
  const float* g;          // DGRAD / WGRAD: d loss / d z [nb][cout][H][W]
  const float* w;          // [cout][cin][taps]
  const float* bias;       // FWD epilogue, nullable
  float* out;
  const float* add;        // DGRAD epilogue, nullable: out = acc + add (where mask > 0, when a mask is given)
  const float* mask;
  const float* elu_y;      // DGRAD epilogue, nullable: acc *= ELU'(z) from ELU(z)
  const int32_t* action;   // [B][act_steps]; the virtual channel of sample bb is action[bb % B][act_t0 + bb / B] / num_actions
  int32_t nb, B, cin, creal, cout, elu, relu, act_steps, act_t0, num_actions;      // elu, relu: FWD epilogue flags
  // the geometry: a ksize x ksize kernel (taps = ksize^2) at `stride`, `pad` zeros around the input board Hin x Win,
  // the output board H x W.  All of it is wave-uniform.
  int32_t ksize, taps, stride, pad, Hin, Win, H, W;
  RtnDiv by_ksize, by_taps, by_stride;
  int32_t M, N, K, kchunk, nchunks, tiles_m, tiles_n;
};

struct RtnPos { int32_t bb, py, px, rem; };
MZX_HD inline RtnPos rtn_pos(int pos, int h, int w) {
  const int hw = h * w;
  RtnPos s;
  s.bb = pos / hw;
  s.rem = pos - s.bb * hw;
  s.py = s.rem / w;
  s.px = s.rem - s.py * w;
  return s;
}
// the input of channel ci that output position s reads through `tap` (zero in the padding, the action plane included)
MZX_HD inline float rtn_im2col(const RtnGemm& p, const RtnPos& s, int ci, int tap) {
  const int ky = rtn_div(tap, p.by_ksize), kx = tap - ky * p.ksize;
  const int y = s.py * p.stride - p.pad + ky, x = s.px * p.stride - p.pad + kx;
  if (y < 0 || y >= p.Hin || x < 0 || x >= p.Win) return 0.f;
  if (ci >= p.creal) return (float)p.action[(int64_t)(s.bb % p.B) * p.act_steps + p.act_t0 + s.bb / p.B] / (float)p.num_actions;
  return p.x[(((int64_t)s.bb * p.creal + ci) * p.Hin + y) * p.Win + x];
}
// A[m][k]; `row`: FWD the output position m, DGRAD the INPUT position m
template <int MODE>
MZX_HD inline float rtn_a(const RtnGemm& p, int m, int k, const RtnPos& row) {
  if (m >= p.M || k >= p.K) return 0.f;
  if (MODE == RTN_WGRAD) {
    const int hw = p.H * p.W, bb = k / hw;
    return p.g[((int64_t)bb * p.cout + m) * hw + (k - bb * hw)];
  }
  const int c = rtn_div(k, p.by_taps), tap = k - c * p.taps;
  if (MODE == RTN_FWD) return rtn_im2col(p, row, c, tap);
  // DGRAD: the tap contributes where (y + pad - ky, x + pad - kx) is a multiple of the stride whose quotient is on the output board
  const int ky = rtn_div(tap, p.by_ksize), kx = tap - ky * p.ksize;
  const int ty = row.py + p.pad - ky, tx = row.px + p.pad - kx;
  if (ty < 0 || tx < 0) return 0.f;
  const int oy = rtn_div(ty, p.by_stride), ox = rtn_div(tx, p.by_stride);
  if (oy * p.stride != ty || ox * p.stride != tx || oy >= p.H || ox >= p.W) return 0.f;
  return p.g[(((int64_t)row.bb * p.cout + c) * p.H + oy) * p.W + ox];
}
template <int MODE>
MZX_HD inline float rtn_b(const RtnGemm& p, int k, int n) {
  if (n >= p.N || k >= p.K) return 0.f;
  if (MODE == RTN_FWD) return p.w[(int64_t)n * p.K + k];
  if (MODE == RTN_DGRAD) {
    const int co = rtn_div(k, p.by_taps), tap = k - co * p.taps;
    return p.w[((int64_t)co * p.cin + n) * p.taps + tap];
  }
  const int ci = rtn_div(n, p.by_taps), tap = n - ci * p.taps;      // (n is fixed per lane: hoisted out of the K loop)
  return rtn_im2col(p, rtn_pos(k, p.H, p.W), ci, tap);
}
template <int MODE>
MZX_HD inline void rtn_store(const RtnGemm& p, int m, int n, int chunk, float v) {
  if (m >= p.M || n >= p.N) return;
  if (MODE == RTN_WGRAD) { p.out[((int64_t)chunk * p.M + m) * p.N + n] = v; return; }
  if (MODE == RTN_FWD) {
    const RtnPos s = rtn_pos(m, p.H, p.W);
    if (p.bias) v += p.bias[n];
    if (p.elu) v = mzx_elu(v);
    if (p.relu) v = fmaxf(v, 0.f);
    p.out[((int64_t)s.bb * p.cout + n) * (p.H * p.W) + s.rem] = v;
    return;
  }
  const RtnPos s = rtn_pos(m, p.Hin, p.Win);
  const int64_t at = ((int64_t)s.bb * p.creal + n) * (p.Hin * p.Win) + s.rem;
  if (p.elu_y) { const float a = p.elu_y[at]; v *= (a > 0.f ? 1.0f : a + 1.0f); }
  if (p.add && (!p.mask || p.mask[at] > 0.f)) v += p.add[at];
  p.out[at] = v;
}

#ifndef MZX_HOSTCHECK
typedef float rtn_f32x4 __attribute__((ext_vector_type(4)));
#endif

// a wavefront per (chunk, 16 x 16 tile).  WIDE = false: four binary32 accumulator chains over the whole of K, joined
// (0 + 1) + (2 + 3): they hide the MFMA's dependent latency, and four short sums joined at the end round less than one long
// one.  WIDE = true is what a network with a downsample stem runs, every GEMM of its step: its chain of BatchNorm layers is
// several times as deep (eight more blocks before the representation tower), and what the binary32 chains round away
// reaches the first blocks' gradients amplified by every 1 / sigma on the way -- so there every MFMA starts from zero (four
// products in binary32) and its result is added to a binary64 accumulator, rounded once at the end, like every other long
// sum of this file.  The serial build keeps its two orders: one fmaf chain over K, or per 16 values of k four 4-term chains
// added to a double.
template <int MODE, bool WIDE>
struct RtnGemmBody {
  RtnGemm p;
  MZX_HD size_t size() const { return (size_t)p.tiles_m * p.tiles_n * p.nchunks; }
  MZX_WAVE_FN void operator()(size_t item, int lane) const {
    const int tiles = p.tiles_m * p.tiles_n;
    const int chunk = (int)(item / tiles), tile = (int)(item % tiles);
    const int m0 = (tile / p.tiles_n) * 16, n0 = (tile % p.tiles_n) * 16;
    const int k0 = chunk * p.kchunk;
    const int k1 = (p.K - k0 < p.kchunk) ? p.K : k0 + p.kchunk;
#ifdef MZX_HOSTCHECK
    for (int i = 0; i < 16; ++i) {
      const int m = m0 + i;
      if (m >= p.M) break;
      const RtnPos row = row_of(m);
      for (int j = 0; j < 16; ++j) {
        const int n = n0 + j;
        if (n >= p.N) break;
        float acc = 0.f;
        double wide = 0.0;
        for (int k = k0; k < k1; k += 16) {
          float t[4] = {0.f, 0.f, 0.f, 0.f};
          for (int c = 0; c < 4; ++c) {
            float& sum = WIDE ? t[c] : acc;
            for (int kc = k + 4 * c; kc < k + 4 * c + 4 && kc < k1; ++kc) sum = fmaf(rtn_a<MODE>(p, m, kc, row), rtn_b<MODE>(p, kc, n), sum);
          }
          if (WIDE) for (int c = 0; c < 4; ++c) wide += (double)t[c];
        }
        rtn_store<MODE>(p, m, n, chunk, WIDE ? (float)wide : acc);
      }
    }
#else
    const int r = lane & 15, q = lane >> 4;
    const int m = m0 + r, n = n0 + r;
    const RtnPos row = m >= p.M ? RtnPos{0, 0, 0, 0} : row_of(m);
    const rtn_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    rtn_f32x4 acc[4] = {zero, zero, zero, zero};
    double wide[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = k0; k < k1; k += 16) {
      float a[4], b[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kc = k + 4 * c + q;
        a[c] = kc < k1 ? rtn_a<MODE>(p, m, kc, row) : 0.f;
        b[c] = kc < k1 ? rtn_b<MODE>(p, kc, n) : 0.f;
      }
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c], b[c], WIDE ? zero : acc[c], 0, 0, 0);
      if (WIDE) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) wide[i] += (double)acc[c][i];
      }
    }
    const rtn_f32x4 joined = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) rtn_store<MODE>(p, m0 + 4 * q + i, n, chunk, WIDE ? (float)wide[i] : joined[i]);
#endif
  }
  // the position of row m for the two modes whose rows are positions
  MZX_HD RtnPos row_of(int m) const {
    if (MODE == RTN_WGRAD) return RtnPos{0, 0, 0, 0};
    return MODE == RTN_DGRAD ? rtn_pos(m, p.Hin, p.Win) : rtn_pos(m, p.H, p.W);
  }
};

// out[e] = sum over chunks, in increasing order
struct RtnWgradFinishOp {
  const float* partial;
  float* out;
  int32_t elements, nchunks;
  MZX_HD size_t size() const { return (size_t)elements; }
  MZX_HD void operator()(size_t e) const {
    double acc = partial[e];
    for (int c = 1; c < nchunks; ++c) acc += (double)partial[(size_t)c * elements + e];
    out[e] = (float)acc;
  }
};

// d loss / d bias[n] = sum over samples and the board of dz: a wavefront per channel, a fixed order
struct RtnBiasGradBody {
  const float* dz;
  float* out;
  int32_t nb, cout, hw;
  MZX_HD size_t size() const { return (size_t)cout; }
  MZX_WAVE_FN void operator()(size_t n, int lane) const {
    double acc = 0.0;
    const int total = nb * hw;
    for (int i = lane; i < total; i += WAVE_LANES) {
      const int bb = i / hw;
      acc += (double)dz[((int64_t)bb * cout + (int64_t)n) * hw + (i - bb * hw)];
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) out[n] = (float)acc;
  }
};

struct RtnFillOp {
  float* y;
  int64_t n;
  float v;
  MZX_HD size_t size() const { return (size_t)n; }
  MZX_HD void operator()(size_t i) const { y[i] = v; }
};

// out = g where the layer's ReLU passed (y nullable: a copy): d loss / d z of a stem convolution without BatchNorm
struct RtnMaskCopyOp {
  const float* g;
  const float* y;
  float* out;
  int64_t n;
  MZX_HD size_t size() const { return (size_t)n; }
  MZX_HD void operator()(size_t i) const { out[i] = (!y || y[i] > 0.f) ? g[i] : 0.f; }
};

// ------------------------------------------------------------------------------------------------ the pools of the stems
// Element kernels in gather form: an output element reads its window, an input element sums -- in increasing window order
// (row-major over the output board) -- the gradients of the windows that contain it (the averages) or chose it (the maximum).
//   OP_POOL           AvgPool2d(3, 2, 1): count_include_pad, and no window reaches past the padded board: the divisor is 9
//   OP_MAXPOOL        MaxPool2d(3, 2): no padding; the gradient goes to the FIRST maximum in row-major window order (torch's
//                     CPU kernel keeps it; windows of ReLU outputs tie at 0.0 all the time)
//   OP_ADAPTIVE_POOL  AdaptiveAvgPool2d: window i spans floor(i in / out) .. ceil((i + 1) in / out), overlapping when out > in

struct RtnPool {
  const float* x;          // the pool's input [planes][Hin][Win] (backward: the maximum is found again)
  const float* g;          // backward: d loss / d output [planes][H][W]
  float* out;              // forward: [planes][H][W]; backward: d loss / d input [planes][Hin][Win]
  int32_t kind, planes, Hin, Win, H, W;
};
MZX_HD inline int rtn_adaptive_lo(int i, int in, int out) { return (i * in) / out; }
MZX_HD inline int rtn_adaptive_hi(int i, int in, int out) { return ((i + 1) * in + out - 1) / out; }
// the first maximum of the 3 x 3 window at (2 oy, 2 ox), as an index into the plane
MZX_HD inline int rtn_maxpool_at(const float* plane, int win, int oy, int ox, float* value) {
  int at = (2 * oy) * win + 2 * ox;
  float best = plane[at];
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const int k = (2 * oy + ky) * win + 2 * ox + kx;
      const float v = plane[k];
      if (v > best) { best = v; at = k; }
    }
  if (value) *value = best;
  return at;
}
struct RtnPoolFwdOp {
  RtnPool p;
  MZX_HD size_t size() const { return (size_t)p.planes * p.H * p.W; }
  MZX_HD void operator()(size_t i) const {
    const int hw = p.H * p.W;
    const int64_t plane = (int64_t)(i / hw);
    const int rem = (int)(i - (size_t)plane * hw), oy = rem / p.W, ox = rem - oy * p.W;
    const float* x = p.x + plane * p.Hin * p.Win;
    float v = 0.f;
    if (p.kind == OP_MAXPOOL) {
      rtn_maxpool_at(x, p.Win, oy, ox, &v);
    } else if (p.kind == OP_POOL) {
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          const int y = 2 * oy - 1 + ky, xx = 2 * ox - 1 + kx;
          if (y >= 0 && y < p.Hin && xx >= 0 && xx < p.Win) v += x[y * p.Win + xx];
        }
      v /= 9.0f;
    } else {
      const int y0 = rtn_adaptive_lo(oy, p.Hin, p.H), y1 = rtn_adaptive_hi(oy, p.Hin, p.H);
      const int x0 = rtn_adaptive_lo(ox, p.Win, p.W), x1 = rtn_adaptive_hi(ox, p.Win, p.W);
      for (int y = y0; y < y1; ++y)
        for (int xx = x0; xx < x1; ++xx) v += x[y * p.Win + xx];
      v /= (float)((y1 - y0) * (x1 - x0));
    }
    p.out[i] = v;
  }
};
struct RtnPoolBwdOp {
  RtnPool p;
  MZX_HD size_t size() const { return (size_t)p.planes * p.Hin * p.Win; }
  MZX_HD void operator()(size_t i) const {
    const int hw = p.Hin * p.Win;
    const int64_t plane = (int64_t)(i / hw);
    const int rem = (int)(i - (size_t)plane * hw), iy = rem / p.Win, ix = rem - iy * p.Win;
    const float* g = p.g + plane * p.H * p.W;
    float v = 0.f;
    if (p.kind == OP_MAXPOOL) {          // windows oy with 2 oy <= iy <= 2 oy + 2
      const float* x = p.x + plane * hw;
      const int oy0 = iy >= 2 ? (iy - 1) / 2 : 0, ox0 = ix >= 2 ? (ix - 1) / 2 : 0;
      for (int oy = oy0; oy <= iy / 2 && oy < p.H; ++oy)
        for (int ox = ox0; ox <= ix / 2 && ox < p.W; ++ox)
          if (rtn_maxpool_at(x, p.Win, oy, ox, nullptr) == rem) v += g[oy * p.W + ox];
    } else if (p.kind == OP_POOL) {      // windows oy with 2 oy - 1 <= iy <= 2 oy + 1
      for (int oy = iy / 2; oy <= (iy + 1) / 2 && oy < p.H; ++oy)
        for (int ox = ix / 2; ox <= (ix + 1) / 2 && ox < p.W; ++ox) v += g[oy * p.W + ox] / 9.0f;
    } else {
      for (int oy = 0; oy < p.H; ++oy) {
        const int y0 = rtn_adaptive_lo(oy, p.Hin, p.H), y1 = rtn_adaptive_hi(oy, p.Hin, p.H);
        if (iy < y0 || iy >= y1) continue;
        for (int ox = 0; ox < p.W; ++ox) {
          const int x0 = rtn_adaptive_lo(ox, p.Win, p.W), x1 = rtn_adaptive_hi(ox, p.Win, p.W);
          if (ix >= x0 && ix < x1) v += g[oy * p.W + ox] / (float)((y1 - y0) * (x1 - x0));
        }
      }
    }
    p.out[i] = v;
  }
};

// ------------------------------------------------------------------------------------------------ BatchNorm, training mode

// S, the type of the batch statistics, the backward sums and the arithmetic of normalise / dz: float, or double in a network
// with a downsample stem (WIDE).  A mean or 1 / sigma rounded to binary32 shifts or scales a whole channel by one correlated
// error, which the sums of the next layers do not average away; behind nineteen BatchNorm layers that is what the gradients'
// error is made of.  The running statistics fold the binary32-rounded batch statistics in both.
template <class S>
struct RtnBn {
  const float* z;          // [napps][B][C][HW]
  const float* y;          // the layer's output (after residual and ReLU): the ReLU mask of the backward pass
  const float* res;        // nullable, [napps][B][C][HW]
  const float* g;          // d loss / d y
  float* out;              // forward: y; backward: dz
  const float* gamma;
  const float* beta;
  S* saved;                // [napps][3][C]: mean, 1 / sigma, biased variance
  S* sums;                 // [napps][2][C]: sum g, sum g x^
  float* running;          // [2][C]: running_mean, running_var of the statistics output
  float* dgamma;
  float* dbeta;
  int32_t napps, B, C, HW;
};

template <class S>
struct RtnBnStatBody {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.napps * p.C; }
  MZX_WAVE_FN void operator()(size_t item, int lane) const {
    const int app = (int)(item / p.C), c = (int)(item % p.C);
    const int n = p.B * p.HW;
    const float* z = p.z + ((int64_t)app * p.B * p.C + c) * p.HW;
    // binary64 accumulators (the reference's CPU BatchNorm sums in binary64 too): the statistics are rounded once
    double s = 0.0;
    for (int i = lane; i < n; i += WAVE_LANES) { const int b = i / p.HW; s += (double)z[(int64_t)b * p.C * p.HW + (i - b * p.HW)]; }
    const double mean = wave_sum_f64(s) / (double)n;
    double s2 = 0.0;
    for (int i = lane; i < n; i += WAVE_LANES) {
      const int b = i / p.HW;
      const double d = (double)z[(int64_t)b * p.C * p.HW + (i - b * p.HW)] - mean;
      s2 += d * d;
    }
    const double var = wave_sum_f64(s2) / (double)n;
    if (lane == 0) {
      S* sv = p.saved + (int64_t)app * 3 * p.C;
      sv[c] = (S)mean; sv[p.C + c] = (S)(1.0 / sqrt(var + (double)RTN_BN_EPS)); sv[2 * p.C + c] = (S)var;
    }
  }
};

// running <- 0.9 running + 0.1 batch (the variance unbiased), the applications in forward order; the batch statistics enter
// rounded to binary32, whatever S keeps
template <class S>
struct RtnBnFoldOp {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.C; }
  MZX_HD void operator()(size_t c) const {
    const double n = (double)p.B * p.HW;
    double rm = p.running[c], rv = p.running[p.C + c];
    for (int app = 0; app < p.napps; ++app) {
      const S* sv = p.saved + (int64_t)app * 3 * p.C;
      const float mean = (float)sv[c], var = (float)sv[2 * p.C + c];
      rm = (double)(float)(RTN_BN_MOMENTUM * (double)mean + (1.0 - RTN_BN_MOMENTUM) * rm);
      rv = (double)(float)(RTN_BN_MOMENTUM * ((double)var * n / (n - 1.0)) + (1.0 - RTN_BN_MOMENTUM) * rv);
    }
    p.running[c] = (float)rm; p.running[p.C + c] = (float)rv;
  }
};

template <class S>
struct RtnBnApplyOp {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.napps * p.B * p.C * p.HW; }
  MZX_HD void operator()(size_t i) const {
    const int c = (int)((i / p.HW) % p.C), app = (int)(i / ((size_t)p.B * p.C * p.HW));
    const S* sv = p.saved + (int64_t)app * 3 * p.C;
    S v = ((S)p.z[i] - sv[c]) * sv[p.C + c] * (S)p.gamma[c] + (S)p.beta[c];
    if (p.res) v += (S)p.res[i];
    p.out[i] = fmaxf((float)v, 0.f);
  }
};

template <class S>
struct RtnBnSumsBody {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.napps * p.C; }
  MZX_WAVE_FN void operator()(size_t item, int lane) const {
    const int app = (int)(item / p.C), c = (int)(item % p.C);
    const int n = p.B * p.HW;
    const int64_t base = ((int64_t)app * p.B * p.C + c) * p.HW;
    const S* sv = p.saved + (int64_t)app * 3 * p.C;
    const S mean = sv[c], inv = sv[p.C + c];
    double sg = 0.0, sgx = 0.0;
    for (int i = lane; i < n; i += WAVE_LANES) {
      const int b = i / p.HW;
      const int64_t at = base + (int64_t)b * p.C * p.HW + (i - b * p.HW);
      const S g = p.y[at] > 0.f ? (S)p.g[at] : (S)0;
      sg += (double)g;
      sgx += (double)g * (double)(((S)p.z[at] - mean) * inv);
    }
    sg = wave_sum_f64(sg); sgx = wave_sum_f64(sgx);
    if (lane == 0) { p.sums[(int64_t)app * 2 * p.C + c] = (S)sg; p.sums[(int64_t)app * 2 * p.C + p.C + c] = (S)sgx; }
  }
};

template <class S>
struct RtnBnDzOp {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.napps * p.B * p.C * p.HW; }
  MZX_HD void operator()(size_t i) const {
    const int c = (int)((i / p.HW) % p.C), app = (int)(i / ((size_t)p.B * p.C * p.HW));
    const S* sv = p.saved + (int64_t)app * 3 * p.C;
    const S* sm = p.sums + (int64_t)app * 2 * p.C;
    const S n = (S)(p.B * p.HW);
    const S g = p.y[i] > 0.f ? (S)p.g[i] : (S)0;
    const S xh = ((S)p.z[i] - sv[c]) * sv[p.C + c];
    p.out[i] = (float)((S)p.gamma[c] * sv[p.C + c] * (g - sm[c] / n - xh * (sm[p.C + c] / n)));
  }
};

// d gamma = sum g x^, d beta = sum g, over the applications in increasing order
template <class S>
struct RtnBnParamGradOp {
  RtnBn<S> p;
  MZX_HD size_t size() const { return (size_t)p.C; }
  MZX_HD void operator()(size_t c) const {
    double dg = 0.0, db = 0.0;
    for (int app = 0; app < p.napps; ++app) { db += (double)p.sums[(int64_t)app * 2 * p.C + c]; dg += (double)p.sums[(int64_t)app * 2 * p.C + p.C + c]; }
    p.dgamma[c] = (float)dg; p.dbeta[c] = (float)db;
  }
};

// ------------------------------------------------------------------------------------------------ the state normalisation

struct RtnScale {
  const float* s;          // raw states [groups][len]
  float* out;              // forward: h; backward: d loss / d s
  const float* g1;         // backward: d loss / d h, two sources (the second nullable)
  const float* g2;
  const float* extra;      // backward, nullable: added to d loss / d s (the reward head's share)
  float factor;            // the 0.5 hook, or 1
  int32_t groups, len;
};

// the smaller value, the lower index on a tie: every lane ends with the same pair
MZX_WAVE_FN void rtn_wave_argmin(float& v, int& at) {
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) {
    const float ov = lane_xor(v, o);
    const int oa = lane_xor(at, o);
    if (ov < v || (ov == v && oa < at)) { v = ov; at = oa; }
  }
}
struct RtnScaleStat { float lo, scale; int imin, imax; };
MZX_WAVE_FN RtnScaleStat rtn_scale_stat(const float* s, int len, int lane) {
  float lo = MZX_INF, nhi = MZX_INF;        // nhi: the minimum of -s
  int imin = 0x7fffffff, imax = 0x7fffffff;
  for (int k = lane; k < len; k += WAVE_LANES) {
    const float v = s[k];
    if (v < lo) { lo = v; imin = k; }
    if (-v < nhi) { nhi = -v; imax = k; }
  }
  rtn_wave_argmin(lo, imin);
  rtn_wave_argmin(nhi, imax);
  RtnScaleStat st;
  st.lo = lo; st.imin = imin; st.imax = imax;
  st.scale = -nhi - lo;
  if (st.scale < 1e-5f) st.scale += 1e-5f;
  return st;
}
struct RtnScaleFwdBody {
  RtnScale p;
  MZX_HD size_t size() const { return (size_t)p.groups; }
  MZX_WAVE_FN void operator()(size_t grp, int lane) const {
    const float* s = p.s + (int64_t)grp * p.len;
    const RtnScaleStat st = rtn_scale_stat(s, p.len, lane);
    for (int k = lane; k < p.len; k += WAVE_LANES) p.out[(int64_t)grp * p.len + k] = (s[k] - st.lo) / st.scale;
  }
};
// h = (s - min) / scale, scale = max - min (+ 1e-5): q = g / scale goes to s, -sum q to min, -sum q h to scale
struct RtnScaleBwdBody {
  RtnScale p;
  MZX_HD size_t size() const { return (size_t)p.groups; }
  MZX_WAVE_FN void operator()(size_t grp, int lane) const {
    const int64_t base = (int64_t)grp * p.len;
    const float* s = p.s + base;
    const RtnScaleStat st = rtn_scale_stat(s, p.len, lane);
    double acc_q = 0.0, acc_qh = 0.0;
    for (int k = lane; k < p.len; k += WAVE_LANES) {
      const float gh = (p.g2 ? p.g1[base + k] + p.g2[base + k] : p.g1[base + k]) * p.factor;
      const float q = gh / st.scale;
      acc_q += (double)q;
      acc_qh += (double)q * (double)((s[k] - st.lo) / st.scale);
    }
    const float sum_q = (float)wave_sum_f64(acc_q), sum_qh = (float)wave_sum_f64(acc_qh);
    const float dscale = -sum_qh;
    for (int k = lane; k < p.len; k += WAVE_LANES) {
      const float gh = (p.g2 ? p.g1[base + k] + p.g2[base + k] : p.g1[base + k]) * p.factor;
      float d = gh / st.scale;
      if (k == st.imin) d += -sum_q - dscale;
      if (k == st.imax) d += dscale;
      if (p.extra) d += p.extra[base + k];
      p.out[base + k] = d;
    }
  }
};

// ------------------------------------------------------------------------------------------------ the plan (host)

constexpr int RTN_PLAIN = 100;       // a layer kind beside OpKind: DownSample's strided 3 x 3 convolutions (no BatchNorm, no bias, no ReLU)
inline bool rtn_is_pool(int kind) { return kind == OP_POOL || kind == OP_MAXPOOL || kind == OP_ADAPTIVE_POOL; }

struct RtnLayer {
  // OP_CONV3 (+ BatchNorm [+ residual] + ReLU), OP_CONV1 (bias), OP_LINEAR (bias [+ ELU]); in the stem of a downsample
  // network also RTN_PLAIN, OP_CONVK (bias + ReLU) and the three pools (no weights: y only)
  int kind = 0;
  int32_t cin = 0, creal = 0, cout = 0, elu = 0, relu = 0, has_res = 0;
  // the geometry, a Linear layer's by default: a 1 x 1 kernel on a 1 x 1 board.  Hin x Win -> H x W
  int32_t ksize = 1, taps = 1, stride = 1, pad = 0, Hin = 1, Win = 1, H = 1, W = 1;
  int64_t w = -1, b = -1;            // flat offsets
  BnRef bn;
  int64_t stat = -1;                 // offset of this BatchNorm in the statistics output
  // scratch offsets in floats (saved / sums hold doubles in a stem network); y / dz = -1: the logits / the loss head's gradients
  int64_t z = -1, y = -1, dz = -1, saved = -1, sums = -1;
  int64_t per_app(int B) const { return (int64_t)B * cout * H * W; }
};
enum RtnNetId { RTN_REP, RTN_DYN, RTN_PRED, RTN_REW, RTN_VAL, RTN_POL, RTN_NETS };
struct RtnChain { std::vector<RtnLayer> l; int32_t napps = 0, t0 = 0; };
struct RtnPlan : TrainHeadPlan {      // A, F and the loss head's scratch offsets
  RtnChain net[RTN_NETS];
  int32_t B = 0, steps = 0, C = 0, HW = 0, num_params = 0, stem = 0;
  int64_t state = 0;                 // B * C * HW
  int64_t off_h = 0, off_ghp = 0, off_grs = 0, off_gd = 0, off_ga = 0, off_gb = 0, off_partial = 0, total_floats = 0;
  struct IdleBn { int64_t stat, mean; int32_t channels; };
  std::vector<IdleBn> idle;          // BatchNorms no chain applies (the bypassed representation_network.module.bn of a stem)
};

inline int64_t rtn_stat_floats(const mzx_net* net) {
  int64_t n = 0;
  for (const BnRef& b : net->bns) n += 2 * (int64_t)b.channels;
  return n;
}

inline int rtn_wgrad_chunks(const RtnLayer& L, int napps, int B) {
  const int64_t K = (int64_t)napps * B * L.H * L.W;
  return (int)((K + RTN_KCHUNK - 1) / RTN_KCHUNK);
}

// The chains, sizes and scratch offsets of a step at (B, steps); false (with the limit named) for what the kernels do not run.
inline bool rtn_plan(const mzx_net* net, int32_t B, int32_t steps, bool own_vlog, bool own_rlog, bool own_plog, RtnPlan& P,
                    std::string* why = nullptr) {
  auto no = [&](const char* msg) { if (why) *why = msg; return false; };
  if (!net) return no("null network handle");
  if (net->cfg.network != 1) return no("fully connected networks train through mzx_train_fc_step (residual networks only)");
  const bool stem = net->cfg.downsample != 0;
  if (stem && !net->train_stem) return no("downsample stems (the strided convolutions and pools) are not trained natively");
  if (B < 1 || steps < 1) return no("batch and steps must be positive");
  if (net->cfg.blocks < 1) return no("the training kernels need at least one residual block per network");
  if (net->num_params >= ((int64_t)1 << 30)) return no("too many parameters");
  const int C = net->hc, HW = net->hh * net->hw;
  if ((int64_t)B * HW < 2) return no("BatchNorm in training mode needs more than one value per channel (batch x board >= 2)");
  if ((int64_t)B * steps * (int64_t)(C > net->cfg.action_space_size ? C : net->cfg.action_space_size) * HW >= ((int64_t)1 << 31) ||
      (int64_t)B * net->input_size >= ((int64_t)1 << 31))
    return no("batch x steps too large");
  P = RtnPlan();
  P.B = B; P.steps = steps; P.C = C; P.HW = HW; P.A = net->cfg.action_space_size; P.F = 2 * net->cfg.support_size + 1;
  P.num_params = (int32_t)net->num_params; P.state = (int64_t)B * C * HW; P.stem = stem ? 1 : 0;
  const int napps[RTN_NETS] = {1, steps - 1, steps, steps - 1, steps, steps};
  const int t0[RTN_NETS] = {0, 1, 0, 1, 0, 0};
  for (int n = 0; n < RTN_NETS; ++n) { P.net[n].napps = napps[n]; P.net[n].t0 = t0[n]; }

  bool in_stem = false;              // the operator being cut may be one of the stem's (the head of prog_initial)
  auto layer_of = [&](const OpDesc& d, RtnLayer& L) {
    L.kind = d.kind; L.w = d.w;
    if (in_stem && (d.kind == OP_CONVK || (d.kind == OP_CONV3 && d.bn.channels == 0))) {
      const bool k = d.kind == OP_CONVK;
      if (d.w < 0 || d.use_action || d.res != -100 || (k ? d.b < 0 || !d.relu : d.relu != 0)) return false;
      L.kind = k ? (int)OP_CONVK : RTN_PLAIN; L.b = k ? d.b : -1; L.relu = d.relu;
      L.ksize = k ? d.ksize : 3; L.stride = d.stride; L.pad = k ? d.pad : 1;
      L.cin = L.creal = d.cin; L.cout = d.cout; L.Hin = d.hin; L.Win = d.win; L.H = d.hout; L.W = d.wout;
      L.taps = L.ksize * L.ksize;
      return L.ksize >= 1 && L.stride >= 1 && L.pad >= 0 && L.H >= 1 && L.W >= 1 &&
             L.H == (L.Hin + 2 * L.pad - L.ksize) / L.stride + 1 && L.W == (L.Win + 2 * L.pad - L.ksize) / L.stride + 1;
    }
    if (in_stem && rtn_is_pool(d.kind)) {
      L.w = -1;
      L.cin = L.creal = L.cout = d.cin; L.Hin = d.hin; L.Win = d.win; L.H = d.hout; L.W = d.wout;
      if (L.H < 1 || L.W < 1) return false;
      if (d.kind == OP_POOL) return L.H == (L.Hin - 1) / 2 + 1 && L.W == (L.Win - 1) / 2 + 1;
      if (d.kind == OP_MAXPOOL) return L.Hin >= 3 && L.Win >= 3 && L.H == (L.Hin - 3) / 2 + 1 && L.W == (L.Win - 3) / 2 + 1;
      return true;
    }
    if (d.kind == OP_CONV3) {
      if (d.stride != 1 || !d.relu || d.bn.channels != d.cout || d.w < 0) return false;
      L.cin = d.cin; L.creal = d.use_action ? d.cin - 1 : d.cin; L.cout = d.cout; L.H = d.hin; L.W = d.win; L.taps = 9;
      L.Hin = d.hin; L.Win = d.win; L.ksize = 3; L.pad = 1;
      L.has_res = d.res != -100; L.bn = d.bn;
      int64_t at = 0;
      for (const BnRef& b : net->bns) { if (b.weight == d.bn.weight) { L.stat = at; break; } at += 2 * (int64_t)b.channels; }
      // the statistics output of a BatchNorm is a copy of its [running_mean | running_var] span of the flat buffer
      return L.stat >= 0 && d.bn.var == d.bn.mean + d.bn.channels;
    }
    if (d.kind == OP_CONV1) {
      L.cin = L.creal = d.cin; L.cout = d.cout; L.H = L.Hin = d.hin; L.W = L.Win = d.win; L.b = d.b;
      return d.b >= 0;
    }
    if (d.kind == OP_LINEAR) {
      if (d.use_action || d.w_stride != d.in_features) return false;
      L.cin = L.creal = d.in_features; L.cout = d.out_features; L.elu = d.elu; L.b = d.b;
      return d.b >= 0;
    }
    return false;
  };
  // prog: tower | OP_SCALE | [reward head] | prediction tower | conv1x1 value, conv1x1 policy | value MLP | policy MLP
  auto cut = [&](const std::vector<OpDesc>& prog, int tower, bool reward, bool keep_prediction) {
    size_t i = 0;
    RtnLayer L;
    in_stem = stem && tower == RTN_REP;
    for (; i < prog.size() && (prog[i].kind == OP_CONV3 || (in_stem && (prog[i].kind == OP_CONVK || rtn_is_pool(prog[i].kind)))); ++i) {
      L = RtnLayer();
      if (!layer_of(prog[i], L)) return false;
      P.net[tower].l.push_back(L);
    }
    in_stem = false;
    if (i >= prog.size() || prog[i].kind != OP_SCALE || prog[i].groups_per_sample != C || prog[i].len != HW) return false;
    ++i;
    auto mlp = [&](int id, int out_buf) {
      for (; i < prog.size() && prog[i].kind == OP_LINEAR; ++i) {
        L = RtnLayer();
        if (!layer_of(prog[i], L)) return false;
        if (keep_prediction || id == RTN_REW) P.net[id].l.push_back(L);
        if (prog[i].out == out_buf) { ++i; return true; }
      }
      return false;
    };
    if (reward) {
      if (i >= prog.size() || prog[i].kind != OP_CONV1) return false;
      L = RtnLayer(); if (!layer_of(prog[i], L)) return false; P.net[RTN_REW].l.push_back(L); ++i;
      if (!mlp(RTN_REW, BUF_REWARD)) return false;
    }
    for (; i < prog.size() && prog[i].kind == OP_CONV3; ++i) {
      L = RtnLayer(); if (!layer_of(prog[i], L)) return false;
      if (keep_prediction) P.net[RTN_PRED].l.push_back(L);
    }
    for (int id : {RTN_VAL, RTN_POL}) {
      if (i >= prog.size() || prog[i].kind != OP_CONV1) return false;
      L = RtnLayer(); if (!layer_of(prog[i], L)) return false;
      if (keep_prediction) P.net[id].l.push_back(L);
      ++i;
    }
    if (!mlp(RTN_VAL, BUF_VALUE) || !mlp(RTN_POL, BUF_POLICY)) return false;
    return i == prog.size();
  };
  if (!cut(net->prog_initial, RTN_REP, false, true) || !cut(net->prog_recurrent, RTN_DYN, true, false))
    return no("unexpected operator program");
  // towers: [first convolution] then blocks of two convolutions, the second with the block's input as its residual; in the
  // representation network of a downsample configuration, segments of blocks separated by a geometry-changing operator
  // (a strided or biased convolution, a pool), the first of which reads the observation
  for (int n : {RTN_REP, RTN_DYN, RTN_PRED}) {
    const std::vector<RtnLayer>& l = P.net[n].l;
    if (l.empty() || l.back().cout != C || l.back().H * l.back().W != HW) return no("unexpected operator program");
    for (int i = (int)l.size() - 1; i >= 0;) {
      if (l[i].has_res) {
        if (i < 1 || l[i].kind != OP_CONV3 || l[i - 1].kind != OP_CONV3 || l[i - 1].has_res || (i == 1 && n != RTN_PRED))
          return no("unexpected operator program");
        if (l[i - 1].cin != l[i].cout || l[i - 1].cout != l[i].cout || l[i].cin != l[i].cout || l[i - 1].H != l[i].H || l[i - 1].W != l[i].W)
          return no("unexpected operator program");
        i -= 2;
      } else if (l[i].kind == OP_CONV3) {
        if (i != 0 || n == RTN_PRED) return no("unexpected operator program");
        i -= 1;
      } else {
        if (n != RTN_REP || (i == 0 && rtn_is_pool(l[i].kind))) return no("unexpected operator program");
        i -= 1;
      }
    }
    for (size_t i = 1; i < l.size(); ++i)
      if (l[i].creal != l[i - 1].cout || l[i].Hin != l[i - 1].H || l[i].Win != l[i - 1].W) return no("unexpected operator program");
  }
  if (stem) {
    const std::vector<RtnLayer>& l = P.net[RTN_REP].l;
    if (rtn_is_pool(l[0].kind) || l[0].kind == OP_CONV3 || (int64_t)l[0].cin * l[0].Hin * l[0].Win != net->input_size)
      return no("unexpected operator program");
    for (const RtnLayer& L : l) {
      if (L.kind == OP_CONV3 && (int64_t)B * L.H * L.W < 2)
        return no("BatchNorm in training mode needs more than one value per channel (batch x board >= 2)");
      // the stem's activations (the largest is the first convolution's, B x C/2 x ceil(H/2) x ceil(W/2) in DownSample) and
      // the chunk partials of its weight gradients are indexed with 32-bit positions
      if ((int64_t)B * L.cout * L.H * L.W >= ((int64_t)1 << 31) || (int64_t)B * L.cin * L.Hin * L.Win >= ((int64_t)1 << 31))
        return no("batch x steps too large");
      if (!rtn_is_pool(L.kind) &&
          (((int64_t)B * L.H * L.W + RTN_KCHUNK - 1) / RTN_KCHUNK) * L.cout * L.cin * L.taps >= ((int64_t)1 << 31))
        return no("batch x steps too large");
    }
  }
  // BatchNorms that no chain applies keep their statistics and have zero gradients
  {
    int64_t at = 0;
    for (const BnRef& b : net->bns) {
      bool applied = false;
      for (int n : {RTN_REP, RTN_DYN, RTN_PRED})
        for (const RtnLayer& L : P.net[n].l) applied |= (L.kind == OP_CONV3 && L.stat == at);
      if (!applied) {
        if (b.var != b.mean + b.channels) return no("unexpected operator program");
        P.idle.push_back({at, b.mean, b.channels});
      }
      at += 2 * (int64_t)b.channels;
    }
  }
  if (P.net[RTN_DYN].l[0].creal != C || P.net[RTN_PRED].l[0].cin != C) return no("unexpected operator program");
  for (int n : {RTN_REW, RTN_VAL, RTN_POL})
    if (P.net[n].l.size() < 2 || P.net[n].l[0].cin != C || P.net[n].l.back().cout != (n == RTN_POL ? P.A : P.F))
      return no("unexpected operator program");

  int64_t o = 0;
  auto take = [&](int64_t floats) { const int64_t at = o; o += (floats + 3) & ~(int64_t)3; return at; };
  const int64_t rows = (int64_t)B * steps;
  train_head_take(P, take, rows, own_vlog, own_rlog, own_plog);
  P.off_h = take(steps * P.state); P.off_ghp = take(steps * P.state); P.off_grs = take((steps - 1) * P.state);
  // the two gradient buffers also carry d loss / d y down the stem, whose boards are larger than the hidden state's
  int64_t gbuf = steps * P.state;
  for (const RtnLayer& L : P.net[RTN_REP].l) if (L.per_app(B) > gbuf) gbuf = L.per_app(B);
  P.off_gd = take(P.state); P.off_ga = take(gbuf); P.off_gb = take(gbuf);
  int64_t partial = 0;
  for (int n = 0; n < RTN_NETS; ++n) {
    RtnChain& ch = P.net[n];
    for (size_t i = 0; i < ch.l.size(); ++i) {
      RtnLayer& L = ch.l[i];
      const int64_t all = ch.napps * L.per_app(B);
      const bool head_out = n >= RTN_REW && i + 1 == ch.l.size();
      const int wide = stem ? 2 : 1;      // floats per statistic
      if (L.kind == OP_CONV3) { L.z = take(all); L.saved = take((int64_t)ch.napps * 3 * L.cout * wide); L.sums = take((int64_t)ch.napps * 2 * L.cout * wide); }
      L.y = head_out ? -1 : take(all);
      if (rtn_is_pool(L.kind)) continue;
      L.dz = head_out ? -1 : take(all);
      const int chunks = rtn_wgrad_chunks(L, ch.napps, B);
      if (chunks > 1 && (int64_t)chunks * L.cout * L.cin * L.taps > partial) partial = (int64_t)chunks * L.cout * L.cin * L.taps;
    }
  }
  P.off_partial = take(partial);
  P.total_floats = o;
  return true;
}

// ------------------------------------------------------------------------------------------------ the step (host)

// WIDE: the precision switch of every GEMM and BatchNorm kernel of the step (a network with a downsample stem)
template <bool WIDE>
struct RtnRun {
  typedef typename std::conditional<WIDE, double, float>::type S;
  const RtnPlan* P;
  const float* flat;
  const float* obs;
  const int32_t* action;
  float* scratch;
  float* grad;
  float* stats;
  float* vlog;
  float* rlog;
  float* plog;
  stream_t stream;
  int rc = 0;
  int launched = 0;
  bool dry = false;            // count the launches of a step without making them (no pointer is read)

  template <class F> void go(F f) {
    if (rc) return;
    ++launched;
    if (!dry) rc = f();
  }

  const float* head_grad(int n) const {          // the loss head's gradient rows of the chain's first application
    const RtnPlan& p = *P;
    if (n == RTN_VAL) return scratch + p.off_gv;
    if (n == RTN_POL) return scratch + p.off_gp;
    return scratch + p.off_gr + (int64_t)p.B * p.F;
  }
  float* head_logits(int n) const {
    if (n == RTN_VAL) return vlog;
    if (n == RTN_POL) return plog;
    return rlog + (int64_t)P->B * P->F;
  }
  // the buffers of layer i of chain n, from application `app` on
  float* y_of(int n, size_t i, int app) const {
    const RtnLayer& L = P->net[n].l[i];
    return (L.y < 0 ? head_logits(n) : scratch + L.y) + (int64_t)app * L.per_app(P->B);
  }
  const float* dz_of(int n, size_t i, int app) const {
    const RtnLayer& L = P->net[n].l[i];
    return (L.dz < 0 ? head_grad(n) : scratch + L.dz) + (int64_t)app * L.per_app(P->B);
  }
  // the input of chain n, from application `app` on: observation, h of the step before, h, raw states, tower outputs
  const float* input_of(int n, int app) const {
    const RtnPlan& p = *P;
    switch (n) {
      case RTN_REP: return obs;
      case RTN_DYN: case RTN_PRED: return scratch + p.off_h + (int64_t)app * p.state;
      case RTN_REW: return y_of(RTN_DYN, p.net[RTN_DYN].l.size() - 1, app);
      default: return y_of(RTN_PRED, p.net[RTN_PRED].l.size() - 1, app);
    }
  }
  const float* x_of(int n, size_t i, int app) const { return i == 0 ? input_of(n, app) : y_of(n, i - 1, app); }

  template <int MODE>
  RtnGemm gemm(int n, size_t i, int app, int napps) const {
    const RtnPlan& p = *P;
    const RtnLayer& L = p.net[n].l[i];
    RtnGemm g;
    memset(&g, 0, sizeof(g));
    g.w = flat + L.w;
    g.action = action; g.act_steps = p.steps; g.act_t0 = p.net[n].t0 + app; g.num_actions = p.A;
    g.nb = napps * p.B; g.B = p.B; g.cin = L.cin; g.creal = L.creal; g.cout = L.cout;
    g.ksize = L.ksize; g.taps = L.taps; g.stride = L.stride; g.pad = L.pad; g.Hin = L.Hin; g.Win = L.Win; g.H = L.H; g.W = L.W;
    g.by_ksize = rtn_div_by(L.ksize); g.by_taps = rtn_div_by(L.taps); g.by_stride = rtn_div_by(L.stride);
    const int positions = g.nb * L.H * L.W;
    if (MODE == RTN_FWD) { g.M = positions; g.N = L.cout; g.K = L.cin * L.taps; }
    else if (MODE == RTN_DGRAD) { g.M = g.nb * L.Hin * L.Win; g.N = L.creal; g.K = L.cout * L.taps; }
    else { g.M = L.cout; g.N = L.cin * L.taps; g.K = positions; }
    g.kchunk = MODE == RTN_WGRAD ? RTN_KCHUNK : g.K;
    g.nchunks = MODE == RTN_WGRAD ? (g.K + RTN_KCHUNK - 1) / RTN_KCHUNK : 1;
    g.tiles_m = (g.M + 15) / 16; g.tiles_n = (g.N + 15) / 16;
    return g;
  }
  template <int MODE>
  void launch_gemm(const RtnGemm& g) { go([&] { return launch_waves<RTN_WAVES>(RtnGemmBody<MODE, WIDE>{g}, stream); }); }
  RtnBn<S> bn(int n, size_t i, int app, int napps) const {
    const RtnPlan& p = *P;
    const RtnLayer& L = p.net[n].l[i];
    const int64_t at = (int64_t)app * L.per_app(p.B);
    RtnBn<S> b;
    memset(&b, 0, sizeof(b));
    b.z = scratch + L.z + at; b.y = scratch + L.y + at;
    b.gamma = flat + L.bn.weight; b.beta = flat + L.bn.bias;
    b.saved = (S*)(scratch + L.saved) + (int64_t)app * 3 * L.cout; b.sums = (S*)(scratch + L.sums) + (int64_t)app * 2 * L.cout;
    b.running = stats + L.stat; b.dgamma = grad + L.bn.weight; b.dbeta = grad + L.bn.bias;
    b.napps = napps; b.B = p.B; b.C = L.cout; b.HW = L.H * L.W;
    return b;
  }

  // a pool of the stem: forward (g == nullptr) into its y, or backward from d loss / d y in `g` to d loss / d input in `out`
  void launch_pool(int n, size_t i, int app, int napps, const float* g, float* out) {
    const RtnLayer& L = P->net[n].l[i];
    RtnPool q;
    memset(&q, 0, sizeof(q));
    q.x = x_of(n, i, app); q.g = g; q.out = g ? out : y_of(n, i, app);
    q.kind = L.kind; q.planes = napps * P->B * L.cout; q.Hin = L.Hin; q.Win = L.Win; q.H = L.H; q.W = L.W;
    if (g) go([&] { return launch<256>(RtnPoolBwdOp{q}, stream); });
    else go([&] { return launch<256>(RtnPoolFwdOp{q}, stream); });
  }
  // applications [app, app + napps) of a tower: conv -> batch statistics -> running statistics -> normalise (+ residual) + ReLU
  void tower_forward(int n, int app, int napps) {
    const std::vector<RtnLayer>& l = P->net[n].l;
    for (size_t i = 0; i < l.size(); ++i) {
      if (rtn_is_pool(l[i].kind)) { launch_pool(n, i, app, napps, nullptr, nullptr); continue; }
      RtnGemm g = gemm<RTN_FWD>(n, i, app, napps);
      if (l[i].kind != OP_CONV3) {       // a stem convolution without BatchNorm: z is y
        g.x = x_of(n, i, app); g.out = y_of(n, i, app); g.bias = l[i].b >= 0 ? flat + l[i].b : nullptr; g.relu = l[i].relu;
        launch_gemm<RTN_FWD>(g);
        continue;
      }
      g.x = x_of(n, i, app); g.out = scratch + l[i].z + (int64_t)app * l[i].per_app(P->B);
      launch_gemm<RTN_FWD>(g);
      RtnBn<S> b = bn(n, i, app, napps);
      if (l[i].has_res) b.res = x_of(n, i - 1, app);
      b.out = scratch + l[i].y + (int64_t)app * l[i].per_app(P->B);
      go([&] { return launch_waves<RTN_WAVES>(RtnBnStatBody<S>{b}, stream); });
      go([&] { return launch<64>(RtnBnFoldOp<S>{b}, stream); });
      go([&] { return launch<256>(RtnBnApplyOp<S>{b}, stream); });
    }
  }
  // every application of a head at once: conv1x1 (bias) -> flatten -> Linear (+ ELU) ...
  void head_forward(int n) {
    const RtnChain& ch = P->net[n];
    if (ch.napps < 1) return;
    for (size_t i = 0; i < ch.l.size(); ++i) {
      RtnGemm g = gemm<RTN_FWD>(n, i, 0, ch.napps);
      g.x = x_of(n, i, 0); g.out = y_of(n, i, 0); g.bias = flat + ch.l[i].b; g.elu = ch.l[i].elu;
      launch_gemm<RTN_FWD>(g);
    }
  }
  // every application of a head: d loss / d logits -> dz of every layer -> d loss / d (tower output) in `dest`
  void head_backward(int n, float* dest, bool accumulate) {
    const RtnChain& ch = P->net[n];
    if (ch.napps < 1) return;
    for (size_t i = ch.l.size() - 1;; --i) {
      RtnGemm g = gemm<RTN_DGRAD>(n, i, 0, ch.napps);
      g.g = dz_of(n, i, 0);
      if (i > 0) {
        g.out = scratch + ch.l[i - 1].dz;
        if (ch.l[i - 1].elu) g.elu_y = y_of(n, i - 1, 0);
      } else {
        g.out = dest;
        if (accumulate) g.add = dest;
      }
      launch_gemm<RTN_DGRAD>(g);
      if (i == 0) break;
    }
  }
  void bn_backward(int n, size_t i, int app, int napps, const float* g) {
    RtnBn<S> b = bn(n, i, app, napps);
    b.g = g; b.out = scratch + P->net[n].l[i].dz + (int64_t)app * P->net[n].l[i].per_app(P->B);
    go([&] { return launch_waves<RTN_WAVES>(RtnBnSumsBody<S>{b}, stream); });
    go([&] { return launch<256>(RtnBnDzOp<S>{b}, stream); });
  }
  // applications [app, app + napps) of a tower, from d loss / d (tower output) in `cur` (overwritten; `other` is scratch of
  // the same size) to d loss / d (tower input) in `dest` (nullable: the observation needs none)
  void tower_backward(int n, int app, int napps, float* cur, float* other, float* dest) {
    const std::vector<RtnLayer>& l = P->net[n].l;
    for (int i = (int)l.size() - 1; i >= 0;) {
      if (l[i].has_res) {
        bn_backward(n, i, app, napps, cur);
        RtnGemm g = gemm<RTN_DGRAD>(n, i, app, napps);
        g.g = dz_of(n, i, app); g.out = other;
        launch_gemm<RTN_DGRAD>(g);
        bn_backward(n, i - 1, app, napps, other);
        // the block's input: through its two convolutions, and straight from its output where the ReLU passed
        RtnGemm g1 = gemm<RTN_DGRAD>(n, i - 1, app, napps);
        g1.g = dz_of(n, i - 1, app); g1.out = (i - 1 == 0) ? dest : cur; g1.add = cur; g1.mask = y_of(n, i, app);
        launch_gemm<RTN_DGRAD>(g1);
        i -= 2;
      } else if (l[i].kind == OP_CONV3) {
        bn_backward(n, i, app, napps, cur);
        if (dest) {
          RtnGemm g = gemm<RTN_DGRAD>(n, i, app, napps);
          g.g = dz_of(n, i, app); g.out = dest;
          launch_gemm<RTN_DGRAD>(g);
        }
        i -= 1;
      } else if (rtn_is_pool(l[i].kind)) {
        launch_pool(n, i, app, napps, cur, other);
        float* t = cur; cur = other; other = t;
        i -= 1;
      } else {
        // a stem convolution without BatchNorm: dz = d loss / d y (where its ReLU passed), kept for the weight gradient; the
        // one that reads the observation sends nothing further
        RtnMaskCopyOp m;
        m.g = cur; m.y = l[i].relu ? y_of(n, i, app) : nullptr; m.n = (int64_t)napps * l[i].per_app(P->B);
        m.out = scratch + l[i].dz + (int64_t)app * l[i].per_app(P->B);
        go([&] { return launch<256>(m, stream); });
        if (i > 0) {
          RtnGemm g = gemm<RTN_DGRAD>(n, i, app, napps);
          g.g = dz_of(n, i, app); g.out = cur;
          launch_gemm<RTN_DGRAD>(g);
        }
        i -= 1;
      }
    }
  }
  // the parameter gradients of a chain, every application in one reduction
  void param_grads(int n) {
    const RtnPlan& p = *P;
    const RtnChain& ch = p.net[n];
    if (ch.napps < 1) return;
    for (size_t i = 0; i < ch.l.size(); ++i) {
      const RtnLayer& L = ch.l[i];
      if (rtn_is_pool(L.kind)) continue;
      RtnGemm g = gemm<RTN_WGRAD>(n, i, 0, ch.napps);
      g.x = x_of(n, i, 0); g.g = dz_of(n, i, 0);
      g.out = g.nchunks > 1 ? scratch + p.off_partial : grad + L.w;
      launch_gemm<RTN_WGRAD>(g);
      if (g.nchunks > 1) {
        RtnWgradFinishOp f;
        f.partial = scratch + p.off_partial; f.out = grad + L.w; f.elements = g.M * g.N; f.nchunks = g.nchunks;
        go([&] { return launch<256>(f, stream); });
      }
      if (L.kind == OP_CONV3) {
        const RtnBn<S> b = bn(n, i, 0, ch.napps);
        go([&] { return launch<64>(RtnBnParamGradOp<S>{b}, stream); });
      } else if (L.b >= 0) {
        RtnBiasGradBody bg;
        bg.dz = dz_of(n, i, 0); bg.out = grad + L.b; bg.nb = ch.napps * p.B; bg.cout = L.cout; bg.hw = L.H * L.W;
        go([&] { return launch_waves<RTN_WAVES>(bg, stream); });
      }
    }
  }
  void scale_forward(int t) {
    const RtnPlan& p = *P;
    RtnScale s;
    memset(&s, 0, sizeof(s));
    s.s = t == 0 ? y_of(RTN_REP, p.net[RTN_REP].l.size() - 1, 0) : y_of(RTN_DYN, p.net[RTN_DYN].l.size() - 1, t - 1);
    s.out = scratch + p.off_h + (int64_t)t * p.state;
    s.groups = p.B * p.C; s.len = p.HW;
    go([&] { return launch_waves<RTN_WAVES>(RtnScaleFwdBody{s}, stream); });
  }
  void scale_backward(int t, float* out) {
    const RtnPlan& p = *P;
    RtnScale s;
    memset(&s, 0, sizeof(s));
    s.s = t == 0 ? y_of(RTN_REP, p.net[RTN_REP].l.size() - 1, 0) : y_of(RTN_DYN, p.net[RTN_DYN].l.size() - 1, t - 1);
    s.out = out;
    s.g1 = scratch + p.off_ghp + (int64_t)t * p.state;
    s.g2 = t + 1 < p.steps ? scratch + p.off_gd : nullptr;
    s.extra = t > 0 ? scratch + p.off_grs + (int64_t)(t - 1) * p.state : nullptr;
    s.factor = t > 0 ? 0.5f : 1.0f;
    s.groups = p.B * p.C; s.len = p.HW;
    go([&] { return launch_waves<RTN_WAVES>(RtnScaleBwdBody{s}, stream); });
  }

  // everything before the loss head
  void forward() {
    const RtnPlan& p = *P;
    // the statistics output starts as the running statistics of the flat buffer: one [mean | var] span per BatchNorm
    for (int n : {RTN_REP, RTN_DYN, RTN_PRED})
      for (const RtnLayer& L : p.net[n].l)
        if (L.kind == OP_CONV3) go([&] { return copy_d2d(stats + L.stat, flat + L.bn.mean, sizeof(float) * 2 * L.cout, stream); });
    for (const RtnPlan::IdleBn& b : p.idle)
      go([&] { return copy_d2d(stats + b.stat, flat + b.mean, sizeof(float) * 2 * b.channels, stream); });
    go([&] { RtnFillOp f; f.y = grad; f.n = p.num_params; f.v = 0.f; return launch<256>(f, stream); });
    tower_forward(RTN_REP, 0, 1);
    scale_forward(0);
    for (int t = 1; t < p.steps; ++t) { tower_forward(RTN_DYN, t - 1, 1); scale_forward(t); }
    go([&] { RewardFillOp f; f.y = rlog; f.batch = p.B; f.full_support = p.F; return launch<256>(f, stream); });
    head_forward(RTN_REW);
    tower_forward(RTN_PRED, 0, p.steps);
    head_forward(RTN_VAL);
    head_forward(RTN_POL);
  }
  // everything after it
  void backward() {
    const RtnPlan& p = *P;
    float* ga = scratch + p.off_ga;
    float* gb = scratch + p.off_gb;
    head_backward(RTN_VAL, ga, false);
    head_backward(RTN_POL, ga, true);
    tower_backward(RTN_PRED, 0, p.steps, ga, gb, scratch + p.off_ghp);
    head_backward(RTN_REW, scratch + p.off_grs, false);
    for (int t = p.steps - 1; t >= 0; --t) {
      scale_backward(t, ga);
      if (t > 0) tower_backward(RTN_DYN, t - 1, 1, ga, gb, scratch + p.off_gd);
      else tower_backward(RTN_REP, 0, 1, ga, gb, nullptr);
    }
    for (int n = 0; n < RTN_NETS; ++n) param_grads(n);
  }
};

}  // namespace mzx
