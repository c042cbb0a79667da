// mzx_optim.h -- the optimizer step over the flat parameter buffer (mzx_optim_step, include/mzx.h): torch's Adam and SGD as
// ONE elementwise wave body that visits only the live spans of the buffer.
//
// The host cuts the spans into chunks of at most MZX_OPTIM_CHUNK elements at absolute multiples of that size
// (optim_cut_chunks; the table lives on the device, built once per network); launch_waves gives every chunk a wavefront.
// Inside a chunk: the elements before the first 16-byte boundary one by one, then four at a time (16-byte loads and
// stores, when every array's base is 16-byte aligned), then the rest one by one.  No atomics, no cross-lane step: every
// element is a function of its own p, g and state only, so the serial build (lane 0 of 1) makes the same bits.
// Adam reads p, g, m, v and writes p, m, v: 28 bytes per element; SGD with momentum reads p, g, buf and writes p, buf: 20.
// What lies outside the spans is neither read nor written.
//
// The arithmetic is the definition in include/mzx.h, every operation a binary32 one with gradual underflow, `/` and sqrt
// correctly rounded (hipcc's default for HIP; the build passes -ffp-contract=off, so no product is fused into a sum).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/mzx.h"
#include "mzx_launch.h"
#include "mzx_net.h"
#include "mzx_wave.h"

namespace mzx {

// g' = g + wd * p; just g when wd == 0 (g + 0 * p is not g for an infinite p or g = -0.0)
MZX_HD inline float optim_decayed(float g, float p, float wd) { return wd != 0.f ? g + wd * p : g; }

struct OptimAdam {
  static constexpr int STATES = 2;
  static constexpr bool LOAD1 = true;
  float wd, c1, b2, c2, bc2s, eps, neg_ss;      // c1 = 1 - beta1, c2 = 1 - beta2, rounded from binary64 once
  MZX_HD void operator()(float& p, float g, float& m, float& v) const {
    g = optim_decayed(g, p, wd);
    m = m + (g - m) * c1;
    v = v * b2 + (c2 * g) * g;
    const float den = sqrtf(v) / bc2s + eps;
    p = p + neg_ss * (m / den);
  }
};

struct OptimSgdPlain {      // momentum 0: no state array
  static constexpr int STATES = 0;
  static constexpr bool LOAD1 = false;
  float wd, neg_lr;
  MZX_HD void operator()(float& p, float g, float&, float&) const { p = p + neg_lr * optim_decayed(g, p, wd); }
};

struct OptimSgdFirst {      // the first step with momentum: the buffer does not exist yet (it is written, never read)
  static constexpr int STATES = 1;
  static constexpr bool LOAD1 = false;
  float wd, neg_lr;
  MZX_HD void operator()(float& p, float g, float& buf, float&) const {
    buf = optim_decayed(g, p, wd);
    p = p + neg_lr * buf;
  }
};

struct OptimSgdMomentum {
  static constexpr int STATES = 1;
  static constexpr bool LOAD1 = true;
  float wd, neg_lr, mu;
  MZX_HD void operator()(float& p, float g, float& buf, float&) const {
    buf = buf * mu + optim_decayed(g, p, wd);
    p = p + neg_lr * buf;
  }
};

struct alignas(16) OptimF4 { float v[4]; };

// One chunk of the table per wavefront.
template <class Rule>
struct OptimBody {
  Rule rule;
  float* p;
  const float* g;
  float* s1;
  float* s2;
  const int64_t* chunks;      // [num_chunks][2]: offset, count
  int64_t n;
  int32_t num_chunks;
  int32_t vec;                // every array's base is 16-byte aligned

  MZX_HD size_t size() const { return (size_t)num_chunks; }

  MZX_HD void one(int64_t i) const {
    float pi = p[i], a = 0.f, b = 0.f;
    if (Rule::LOAD1) a = s1[i];
    if (Rule::STATES >= 2) b = s2[i];
    rule(pi, g[i], a, b);
    p[i] = pi;
    if (Rule::STATES >= 1) s1[i] = a;
    if (Rule::STATES >= 2) s2[i] = b;
  }

  MZX_HD void four(int64_t i) const {      // i is a multiple of 4
    OptimF4 pv = *reinterpret_cast<const OptimF4*>(p + i);
    const OptimF4 gv = *reinterpret_cast<const OptimF4*>(g + i);
    OptimF4 av = {{0.f, 0.f, 0.f, 0.f}}, bv = {{0.f, 0.f, 0.f, 0.f}};
    if (Rule::LOAD1) av = *reinterpret_cast<const OptimF4*>(s1 + i);
    if (Rule::STATES >= 2) bv = *reinterpret_cast<const OptimF4*>(s2 + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) rule(pv.v[k], gv.v[k], av.v[k], bv.v[k]);
    *reinterpret_cast<OptimF4*>(p + i) = pv;
    if (Rule::STATES >= 1) *reinterpret_cast<OptimF4*>(s1 + i) = av;
    if (Rule::STATES >= 2) *reinterpret_cast<OptimF4*>(s2 + i) = bv;
  }

  MZX_HD void operator()(size_t item, int lane) const {
    const int64_t off = chunks[2 * item], count = chunks[2 * item + 1];
    if (off < 0 || count < 0 || count > MZX_OPTIM_CHUNK || off > n - count) return;      // (a table that is not this buffer's)
    const int cnt = (int)count;
    const int head = vec ? ((int)((4 - (off & 3)) & 3) < cnt ? (int)((4 - (off & 3)) & 3) : cnt) : cnt;
    const int quads = (cnt - head) / 4;
    const int tail = cnt - head - 4 * quads;
    WAVE_FOR(j, head) one(off + j);
    WAVE_FOR(j, quads) four(off + head + 4 * (int64_t)j);
    WAVE_FOR(j, tail) one(off + head + 4 * quads + j);
  }
};

// The spans of a table in the order given, each cut at the absolute multiples of MZX_OPTIM_CHUNK; empty spans vanish.
// `emit(offset, count)` per chunk -> how many.
template <class Emit>
inline int64_t optim_cut_chunks(const int64_t* spans, int32_t num_spans, Emit emit) {
  int64_t chunks = 0;
  for (int32_t s = 0; s < num_spans; ++s) {
    int64_t off = spans[2 * s];
    const int64_t end = off + spans[2 * s + 1];
    while (off < end) {
      const int64_t stop = std::min(end, (off / MZX_OPTIM_CHUNK + 1) * MZX_OPTIM_CHUNK);
      emit(off, stop - off);
      off = stop;
      ++chunks;
    }
  }
  return chunks;
}

// Every span inside [0, n), no two of them sharing an element.
inline bool optim_spans_ok(const char* who, const int64_t* spans, int32_t num_spans, int64_t n) {
  if (!spans || num_spans < 0 || n < 0) { set_error("%s: null span table / negative sizes", who); return false; }
  std::vector<std::pair<int64_t, int64_t>> live;
  for (int32_t s = 0; s < num_spans; ++s) {
    const int64_t off = spans[2 * s], count = spans[2 * s + 1];
    if (off < 0 || count < 0 || count > n || off > n - count) {
      set_error("%s: span %d (offset %lld, count %lld) lies outside [0, %lld)", who, s, (long long)off, (long long)count, (long long)n);
      return false;
    }
    if (count > 0) live.push_back({off, count});
  }
  std::sort(live.begin(), live.end());
  for (size_t k = 1; k < live.size(); ++k)
    if (live[k - 1].first + live[k - 1].second > live[k].first) {
      set_error("%s: the spans at offsets %lld and %lld overlap", who, (long long)live[k - 1].first, (long long)live[k].first);
      return false;
    }
  return true;
}

// Every refusal of mzx_optim_step; nothing has been launched when this returns MZX_ERR_INVALID.
inline int optim_check(const mzx_optim_io* io) {
  const char* who = "mzx_optim_step";
  if (!io) { set_error("%s: null argument", who); return MZX_ERR_INVALID; }
  if (io->kind != MZX_OPTIM_ADAM && io->kind != MZX_OPTIM_SGD) { set_error("%s: kind is MZX_OPTIM_ADAM or MZX_OPTIM_SGD", who); return MZX_ERR_INVALID; }
  const bool adam = io->kind == MZX_OPTIM_ADAM;
  if (!io->d_param || !io->d_grad || !io->h_spans || !io->d_chunks || (adam && (!io->d_state1 || !io->d_state2))) {
    set_error("%s: missing buffer", who);
    return MZX_ERR_INVALID;
  }
  if (!adam && io->momentum != 0.0 && !io->d_state1) { set_error("%s: momentum %g needs a momentum buffer (d_state1)", who, io->momentum); return MZX_ERR_INVALID; }
  if (io->t < 1) { set_error("%s: step count t = %lld, it starts at 1", who, (long long)io->t); return MZX_ERR_INVALID; }
  if (!optim_spans_ok(who, io->h_spans, io->num_spans, io->n)) return MZX_ERR_INVALID;
  const int64_t chunks = optim_cut_chunks(io->h_spans, io->num_spans, [](int64_t, int64_t) {});
  if (chunks != io->num_chunks) {
    set_error("%s: the spans make %lld chunks, the device table is said to hold %d (mzx_optim_chunks)", who, (long long)chunks, io->num_chunks);
    return MZX_ERR_INVALID;
  }
  return MZX_OK;
}

template <class Rule>
inline int optim_launch_rule(const Rule& rule, const mzx_optim_io* io, stream_t stream) {
  OptimBody<Rule> body;
  body.rule = rule;
  body.p = io->d_param; body.g = io->d_grad;
  body.s1 = Rule::STATES >= 1 ? io->d_state1 : nullptr;
  body.s2 = Rule::STATES >= 2 ? io->d_state2 : nullptr;
  body.chunks = io->d_chunks; body.n = io->n; body.num_chunks = io->num_chunks;
  const uintptr_t bases = (uintptr_t)body.p | (uintptr_t)body.g | (uintptr_t)body.s1 | (uintptr_t)body.s2;
  body.vec = (bases % 16) == 0 ? 1 : 0;
  return launch_waves<4>(body, stream);
}

// The launch of a checked step (optim_check): the binary64 scalars are rounded to binary32 here, once.
inline int optim_launch(const mzx_optim_io* io, stream_t stream) {
  const float wd = (float)io->weight_decay;
  if (io->kind == MZX_OPTIM_ADAM) {
    OptimAdam r;
    r.wd = wd; r.c1 = (float)io->one_minus_beta1; r.b2 = (float)io->beta2; r.c2 = (float)io->one_minus_beta2;
    r.bc2s = (float)io->bias_correction2_sqrt; r.eps = (float)io->eps; r.neg_ss = (float)-io->step_size;
    return optim_launch_rule(r, io, stream);
  }
  const float neg_lr = (float)-io->lr;
  if (io->momentum == 0.0) {
    OptimSgdPlain r;
    r.wd = wd; r.neg_lr = neg_lr;
    return optim_launch_rule(r, io, stream);
  }
  if (io->first_step) {
    OptimSgdFirst r;
    r.wd = wd; r.neg_lr = neg_lr;
    return optim_launch_rule(r, io, stream);
  }
  OptimSgdMomentum r;
  r.wd = wd; r.neg_lr = neg_lr; r.mu = (float)io->momentum;
  return optim_launch_rule(r, io, stream);
}

}  // namespace mzx
