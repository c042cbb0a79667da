// mzx_draws.h -- the random numbers of a self-play move drawn on the device (opt-in: config.device_draws).
//
// The host path (mzx_rng.h) draws the Dirichlet noise of the root, the tie-break words of the search and the action choice
// from one numpy-compatible MT19937 stream per game: field-identical to the reference, and a per-game host loop.  This header
// DEFINES a second set of draws as a pure function of (seed, stream, counter) over a counter-based generator, so that a
// wavefront per game produces them and a numpy / math restatement exists (tests/device_draws_cases.py).  They are not
// numpy's draws, hence opt-in.
//
// Words.  Every word is one of the four of a Philox4x32-10 block (philox4x32_10, mzx_replay.h):
//     key     = (seed lo, seed hi ^ 0x53454C46 "SELF")    -- apart from the replay sampler's and the reanalyse tape's keys
//     counter = (stream, counter lo, counter hi, (purpose << 30) | index)
//   stream: the game's slot in its shard / the tree number of an engine call (u32); counter: a u64 move or call number, the
//   same for every game of one call; purpose: 0 noise, 1 tape, 2 action; index < 2^30.
//   seed: the caller's u64.  SelfPlay passes the ACTOR's seed (its `seed` argument, the number that seeds its games and, on
//   host draws, its streams: config.seed + rank * games for the ranks of a job), so actors that share a configuration draw
//   apart; a BatchedMCTS on its own takes config.seed unless its draw_seed is set.
// Uniforms.  A sequence of uniforms over consecutive blocks index, index + 1, ... is sampler_u53(w[0], w[1]), then
//   sampler_u53(w[2], w[3]) of each block in turn: ((hi << 21) | (lo >> 11)) * 2^-53, in [0, 1).
// Tape (purpose 1).  Word 4b + j of a game's row is word j of block index = b: a longer tape under the same (stream,
//   counter) begins with the shorter one (that is what the tape-overflow retry asks for).
// Noise (purpose 0).  Child j < n of a root has a sub-stream of its own, index = (j << 14) | block, block = 0, 1, ...
//   (j < 2^16; the block number wraps at 2^14, i.e. after 32 768 uniforms of ONE element, which no rejection loop reaches).
//   g_j = standard_gamma(alpha) by the algorithm of Mt19937::standard_gamma / gauss_polar / standard_exponential of
//   mzx_rng.h, operation for operation, with next_double() replaced by the sub-stream's next uniform and the cached-gaussian
//   flag clear at the start of every element.  sum = the left-to-right binary64 sum g_0 + ... + g_{n-1};
//   noise_j = g_j / sum for j < n, 0.0 for j >= n.  A row whose sum is 0 or not finite gets 1.0 / n in its first n
//   entries: with alpha >= 0.1 (every shipped configuration has 0.25 or 0.3) a gamma variate is 0 only below
//   u^(1/alpha) underflow, u < 1e-30, which a 53-bit uniform other than exactly 0 never is -- not reachable in practice.
//   n = the number of entries >= 0 of the legal row, or the caller's n (continued searches).
// Action (purpose 2, index 0).  One uniform u (the first of the block); n legal children in legal order with visit counts
//   c_j.  Temperature 0: the first maximum of c.  +inf: position min(n - 1, floor(u * n)).  Otherwise w_j =
//   pow_table[row(T)][c_j] (the caller's table of numpy's own powers, as mzx_selfplay_select takes it), P_j the inclusive
//   left-to-right binary64 prefix, t = u * P_{n-1}: the smallest j with P_j > t; if there is none the last j with w_j > 0
//   (position 0 when no weight is positive).  Output: the action legal[j].  Adds, multiplies and compares only: both builds
//   and numpy agree bit for bit.
//
// The device's log / exp / pow / sqrt are not glibc's: tape and action are bit-exact everywhere, the noise is bit-exact in
// the serial build (same libm as Python's math) and within 1e-12 relative on the device (tests/test_gpu_device_draws.py).
#pragma once
#include "mzx_platform.h"
#include "mzx_replay.h"
#include "mzx_wave.h"

namespace mzx {

constexpr uint32_t SELFPLAY_DRAWS_KEY = 0x53454C46u;
constexpr int DRAWS_MAX_ACTIONS = 4096;          // (mzx_selfplay_select's limit; the sub-stream index holds 2^16)
constexpr uint32_t DRAW_NOISE = 0, DRAW_TAPE = 1, DRAW_ACTION = 2;

// (seed, stream, counter) of one game
struct DrawKey {
  uint32_t k0, k1, stream, c_lo, c_hi;
  MZX_HD void block(uint32_t purpose, uint32_t index, uint32_t w[4]) const {
    philox4x32_10(stream, c_lo, c_hi, (purpose << 30) | index, k0, k1, w);
  }
};
MZX_HD inline DrawKey draw_key(uint64_t seed, uint64_t counter, uint32_t stream) {
  DrawKey k;
  k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32) ^ SELFPLAY_DRAWS_KEY;
  k.stream = stream; k.c_lo = (uint32_t)counter; k.c_hi = (uint32_t)(counter >> 32);
  return k;
}

// the uniforms of one root child: two per block; carries the cached gaussian of legacy_gauss
struct DrawUniforms {
  DrawKey key;
  uint32_t base, blocks;
  double second, gauss;
  int have_second, has_gauss;

  MZX_HD DrawUniforms(const DrawKey& k, uint32_t child)
      : key(k), base(child << 14), blocks(0), second(0.0), gauss(0.0), have_second(0), has_gauss(0) {}
  MZX_HD double next() {
    if (have_second) { have_second = 0; return second; }
    uint32_t w[4];
    key.block(DRAW_NOISE, base | (blocks & 0x3FFFu), w);
    ++blocks;
    second = sampler_u53(w[2], w[3]);
    have_second = 1;
    return sampler_u53(w[0], w[1]);
  }
  MZX_HD double standard_exponential() { return -log(1.0 - next()); }
  MZX_HD double gauss_polar() {
    if (has_gauss) {
      const double t = gauss;
      gauss = 0.0;
      has_gauss = 0;
      return t;
    }
    double f, x1, x2, r2;
    do {
      x1 = 2.0 * next() - 1.0;
      x2 = 2.0 * next() - 1.0;
      r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    f = sqrt(-2.0 * log(r2) / r2);
    gauss = f * x1;
    has_gauss = 1;
    return f * x2;
  }
  MZX_HD double standard_gamma(double shape) {
    double b, c, U, V, X, Y;
    if (shape == 1.0) return standard_exponential();
    if (shape == 0.0) return 0.0;
    if (shape < 1.0) {
      for (;;) {
        U = next();
        V = standard_exponential();
        if (U <= 1.0 - shape) {
          X = pow(U, 1. / shape);
          if (X <= V) return X;
        } else {
          Y = -log((1 - U) / shape);
          X = pow(1.0 - shape + shape * Y, 1. / shape);
          if (X <= (V + Y)) return X;
        }
      }
    }
    b = shape - 1. / 3.;
    c = 1. / sqrt(9 * b);
    for (;;) {
      do {
        X = gauss_polar();
        V = 1.0 + c * X;
      } while (V <= 0.0);
      V = V * V * V;
      U = next();
      if (U < 1.0 - 0.0331 * (X * X) * (X * X)) return (b * V);
      if (log(U) < 0.5 * X * X + b * (1. - V + log(V))) return (b * V);
    }
  }
};

// g_j of child j
MZX_HD inline double draw_gamma(const DrawKey& k, int child, double alpha) {
  DrawUniforms u(k, (uint32_t)child);
  return u.standard_gamma(alpha);
}
// block b of the tape: words 4b .. 4b + 3
MZX_HD inline void draw_tape_block(const DrawKey& k, int b, uint32_t w[4]) { k.block(DRAW_TAPE, (uint32_t)b, w); }
// the action uniform
MZX_HD inline double draw_action_uniform(const DrawKey& k) {
  uint32_t w[4];
  k.block(DRAW_ACTION, 0u, w);
  return sampler_u53(w[0], w[1]);
}
// the legal actions of a padded row
MZX_HD inline int draw_count_legal(const int32_t* legal, int A) {
  int n = 0;
  for (int j = 0; j < A; ++j) n += legal[j] >= 0 ? 1 : 0;
  return n;
}

struct SelfplayDrawsParams {
  uint64_t seed, counter;
  const int32_t* streams;       // [B] nullable: first_stream + k
  const int32_t* legal;         // [B][A] nullable: n comes from n_rows
  const int32_t* n_rows;        // [B]
  double* noise;                // [B][A] nullable: no noise
  uint32_t* tape;               // [B][tape_words]
  double alpha;
  int32_t first_stream, B, A, tape_words;

  MZX_HD DrawKey key(size_t e) const {
    return draw_key(seed, counter, (uint32_t)(streams ? streams[e] : first_stream + (int32_t)e));
  }
};

// Noise and tape of one game: launch_waves<SAMPLER_WAVES>, a wavefront per game, a lane per child (the rejection loops
// diverge per lane; every lane then takes the same left-to-right sum out of the 64 registers) and per tape block.  The
// legal row is counted lane-strided and reduced over the wave (an integer sum: the same n in both builds).
struct SelfplayDrawsBody {
  SelfplayDrawsParams p;
  MZX_HD size_t size() const { return (size_t)p.B; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    const DrawKey key = p.key(e);
    const int A = p.A;
    if (p.noise) {
      int n;                                             // (the same in every lane)
      if (p.legal) {
        const int32_t* __restrict__ row = p.legal + e * (size_t)A;
        int32_t mine = 0;
        WAVE_FOR(j, A) mine += row[j] >= 0 ? 1 : 0;
        n = wave_sum_i32(mine);
      } else {
        n = p.n_rows[e];
      }
      n = n < 0 ? 0 : (n > A ? A : n);
      double* __restrict__ out = p.noise + e * (size_t)A;
      double sum = 0.0;
      for (int c0 = 0; c0 < n; c0 += WAVE_LANES) {
        const int j = c0 + lane;
        double g = 0.0;
        if (j < n) {
          g = draw_gamma(key, j, p.alpha);
          out[j] = g;
        }
        for (int l = 0; l < WAVE_LANES && c0 + l < n; ++l) sum = sum + lane_value(g, l);
      }
      const bool ok = sum > 0.0 && sum <= 1.7976931348623157e308;
      const double uniform = n > 0 ? 1.0 / (double)n : 0.0;
      WAVE_FOR(j, A) out[j] = j < n ? (ok ? out[j] / sum : uniform) : 0.0;       // (lane j wrote out[j] itself)
    }
    uint32_t* __restrict__ t = p.tape + e * (size_t)p.tape_words;
    WAVE_FOR(b, (p.tape_words + 3) / 4) {
      uint32_t w[4];
      draw_tape_block(key, b, w);
      for (int j = 0; j < 4 && 4 * b + j < p.tape_words; ++j) t[4 * b + j] = w[j];
    }
  }
};

struct SelfplaySelectParams {
  uint64_t seed, counter;
  const int32_t* streams;       // [B] nullable
  const int32_t* legal;         // [B][A]
  const int32_t* visits;        // [B][A] by action
  const double* temperature;    // [B]
  const double* pow_table;      // [num_temperatures][table_stride]
  const double* table_temperatures;
  const double* uniforms;       // [B] nullable (tests): replaces the action uniform
  int64_t* action;              // [B]
  int32_t first_stream, B, A, table_stride, num_temperatures;
};

// The action of one game (the definition above), MZX_HD: the device body's lane 0 and the host's retry path run it.
// A visit count outside the power table counts as weight 0 (the host entry refuses such rows where it can see them).
MZX_HD inline int64_t draw_select_action(const SelfplaySelectParams& p, size_t e) {
  const int A = p.A;
  const int32_t* legal = p.legal + e * (size_t)A;
  const int32_t* vis = p.visits + e * (size_t)A;
  const int n = draw_count_legal(legal, A);
  if (n < 1) return -1;
  // the visit count of child j (an entry that is no action of the space counts 0: nothing outside the row is read)
  auto count = [&](int j) -> int32_t { const int32_t a = legal[j]; return a >= 0 && a < A ? vis[a] : 0; };
  const double T = p.temperature[e];
  int pos = 0;
  if (T == 0.0) {
    int32_t best = count(0);
    for (int j = 1; j < n; ++j) if (count(j) > best) { best = count(j); pos = j; }
    return legal[pos];
  }
  const double u = p.uniforms ? p.uniforms[e]
                              : draw_action_uniform(draw_key(p.seed, p.counter, (uint32_t)(p.streams ? p.streams[e] : p.first_stream + (int32_t)e)));
  if (T == MZX_INF) {
    const double f = floor(u * (double)n);
    pos = f >= 0.0 ? (f < (double)n ? (int)f : n - 1) : 0;
    return legal[pos];
  }
  int row = -1;
  for (int q = 0; q < p.num_temperatures; ++q) if (p.table_temperatures[q] == T) row = q;
  if (row < 0) return -1;
  const double* tab = p.pow_table + (size_t)row * p.table_stride;
  double total = 0.0;
  for (int j = 0; j < n; ++j) {
    const int32_t c = count(j);
    total = total + (c >= 0 && c < p.table_stride ? tab[c] : 0.0);
  }
  const double t = u * total;
  double acc = 0.0;
  int last = 0;
  pos = -1;
  for (int j = 0; j < n; ++j) {
    const int32_t c = count(j);
    const double w = c >= 0 && c < p.table_stride ? tab[c] : 0.0;
    acc = acc + w;
    if (w > 0.0) last = j;
    if (pos < 0 && acc > t) pos = j;
  }
  return legal[pos < 0 ? last : pos];
}

// launch_waves<SAMPLER_WAVES>, one game per wave: the prefix is sequential by definition, lane 0 walks it
struct SelfplaySelectBody {
  SelfplaySelectParams p;
  MZX_HD size_t size() const { return (size_t)p.B; }
  MZX_WAVE_FN void operator()(size_t e, int lane) const {
    if (lane == 0) p.action[e] = draw_select_action(p, e);
  }
};

}  // namespace mzx
