// mzx_train_gemm_ksplit.h -- the GEMM body of the residual trainer (mzx_train_resnet.h, "The three GEMMs") for the shapes that
// have too few output tiles to fill the device but a K long enough to cut: RtnKsplitGemmBody<MODE, WIDE>, a 256-thread
// workgroup per (weight-gradient chunk, 32 x 32 output tile) whose four waves divide K among them.  It serves the same RtnGemm
// descriptor through the same operand functions (rtn_row / rtn_a / rtn_b / rtn_im2col / rtn_store<MODE>) as the other bodies;
// which GEMMs take it is the handle's train_gemm switch and the rule train_gemm_ksplit of mzx_tuning.h.
//
// Work split.  ALL four waves own the whole 32 x 32 tile, as 2 x 2 MFMA tiles of 16 x 16 on v_mfma_f32_16x16x4_f32.  The
// k-groups of 16 of the chunk are dealt round-robin: group g, counted from the chunk's k0, goes to wave g & 3, and a wave takes
// its groups in increasing order.  A wave's dependent chain is a quarter of the wave body's, it issues 16 MFMAs per gathered
// group where the wave body issues 4, and a gathered A or B value feeds two MFMAs.  The wavefront count equals the wave body's
// (four 16 x 16 tiles per workgroup of four waves).  Per MFMA tile a wave keeps the wave body's four accumulator chains (chain
// c of a group takes k + 4 c .. k + 4 c + 3), feeds a ragged last group zeros, never issues a group that starts at or beyond
// the chunk's end, and joins the chains as (0 + 1) + (2 + 3).  WIDE starts every MFMA from zero and adds it to binary64
// accumulators.  Rows, columns and k beyond M, N and the chunk's end are zero operands, and rtn_store drops what lies outside.
//
// Software pipeline.  A lane gathers 2 x 4 A values (rows m0 + 16 t + r, k + 4 c + q) and 2 x 4 B values (k + 4 c + q, columns
// n0 + 16 u + r) per group, with r = lane & 15, q = lane >> 4.  The gathers of the wave's NEXT group (64 further on) are
// requested into a second set of registers before the 16 MFMAs of the current group are issued; a sched_barrier on each side of
// the MFMA block keeps the compiler from moving the loads behind it or the wait for them in front of it, so no MFMA block
// waits on a gather issued just before it.  Hoisted out of the K loop: the RtnPos of the lane's two rows and, for the weight
// gradient, the (ci, tap) of its two columns, once per GEMM; the position of a weight-gradient k, once per group (four per
// lane, each shared by both rows and both columns).
//
// Which operand goes where.  The MFMA hands lane l the results D[4 (l >> 4) + i][l & 15]: neighbouring lanes hold neighbouring
// COLUMNS of D.  The weight gradient's output is contiguous in n, so it issues mfma(A, B) and D = C.  The forward pass and the
// input gradient write [sample][channel][board], contiguous in m, so they issue mfma(B^T, A^T) -- the same 8 + 8 gathered
// values with the operands exchanged -- and hold D = C^T: neighbouring lanes hold neighbouring positions m.  In both cases the
// 16 lanes of a quad row write 16 neighbouring addresses of the output's contiguous axis.
//
// Cross-wave reduction.  Each wave writes its joined 32 x 32 partial to LDS, 4 x 1024 floats = 16 KB (WIDE: doubles, 32 KB), in
// FRAGMENT-MAJOR layout: [wave][slot = (2 t + u) 4 + i][lane], i.e. the wave stores accumulator register i of MFMA tile (t, u) as
// 64 consecutive words.  A D-fragment write is 64 (128 for doubles) consecutive words: no bank conflict.  After ONE
// __syncthreads() thread T sums the four slots 4 (T >> 6) + j, j = 0 .. 3, at lane position T & 63 -- the elements that lane
// T & 63 of every wave holds for MFMA tile T >> 6 -- so a reduction read is 64 consecutive words as well, and the thread that
// stores an element has the lane position the MFMA gave it: the store keeps the coalescing described above.  The order is
// fixed, (w0 + w1) + (w2 + w3), in binary32, or in binary64 rounded once when WIDE.  A wave that got no group (a chunk of fewer
// than four groups) contributes exact zeros and is summed all the same: the order never depends on the shape.  Every wave
// writes all of its 1024 words before the barrier: nothing relies on zeroed LDS.  No atomics: a second call repeats every bit.
// The result is NOT the wave body's bits (K is summed in another order); its contract is the reference gates.
//
// tests/hostcheck build: rtn_serial_ksplit_tile, per output element four per-wave sums -- each over its groups in the serial
// build's per-group order of rtn_serial_tile (one fmaf chain, or four 4-term chains per group added to a double) -- and the
// fixed join.
#pragma once
#include "mzx_train_resnet.h"

namespace mzx {

constexpr int RTK_THREADS = 256;
constexpr int RTK_WAVES = 4;
constexpr int RTK_TILE = 32;          // rows and columns of a workgroup's output tile: 2 x 2 MFMA tiles
constexpr int RTK_GROUP = 16;         // k per group: four MFMAs of four k per MFMA tile
constexpr int RTK_PARTIAL = RTK_TILE * RTK_TILE;      // words of a wave's partial tile in LDS

#ifdef MZX_HOSTCHECK
template <int MODE, bool WIDE>
inline void rtn_serial_ksplit_tile(const RtnGemm& p, int m0, int n0, int chunk, int k0, int k1) {
  for (int i = 0; i < RTK_TILE; ++i) {
    const int m = m0 + i;
    if (m >= p.M) break;
    const RtnPos row = rtn_row<MODE>(p, m);
    for (int j = 0; j < RTK_TILE; ++j) {
      const int n = n0 + j;
      if (n >= p.N) break;
      float acc[RTK_WAVES];
      double wide[RTK_WAVES];
      for (int w = 0; w < RTK_WAVES; ++w) {
        acc[w] = 0.f;
        wide[w] = 0.0;
        for (int k = k0 + RTK_GROUP * w; k < k1; k += RTK_GROUP * RTK_WAVES) {
          float t[4] = {0.f, 0.f, 0.f, 0.f};
          for (int c = 0; c < 4; ++c) {
            float& sum = WIDE ? t[c] : acc[w];
            for (int kc = k + 4 * c; kc < k + 4 * c + 4 && kc < k1; ++kc) sum = fmaf(rtn_a<MODE>(p, m, kc, row), rtn_b<MODE>(p, kc, n), sum);
          }
          if (WIDE) for (int c = 0; c < 4; ++c) wide[w] += (double)t[c];
        }
      }
      rtn_store<MODE>(p, m, n, chunk, WIDE ? (float)((wide[0] + wide[1]) + (wide[2] + wide[3])) : (acc[0] + acc[1]) + (acc[2] + acc[3]));
    }
  }
}
#endif

template <int MODE, bool WIDE>
struct RtnKsplitGemmBody {
  RtnGemm p;
  MZX_HD int tiles_n() const { return (p.N + RTK_TILE - 1) / RTK_TILE; }
  MZX_HD size_t size() const { return (size_t)((p.M + RTK_TILE - 1) / RTK_TILE) * tiles_n() * p.nchunks; }
  MZX_WAVE_FN void operator()(size_t item, int thread) const {
    const int tiles = ((p.M + RTK_TILE - 1) / RTK_TILE) * tiles_n();
    const int chunk = (int)(item / tiles), tile = (int)(item % tiles);
    const int m0 = (tile / tiles_n()) * RTK_TILE, n0 = (tile % tiles_n()) * RTK_TILE;
    const int k0 = chunk * p.kchunk;
    const int k1 = (p.K - k0 < p.kchunk) ? p.K : k0 + p.kchunk;
#ifdef MZX_HOSTCHECK
    (void)thread;
    rtn_serial_ksplit_tile<MODE, WIDE>(p, m0, n0, chunk, k0, k1);
#else
    typedef typename std::conditional<WIDE, double, float>::type S;
    __shared__ S lds[RTK_WAVES][RTK_PARTIAL];
    constexpr bool WGRAD = MODE == RTN_WGRAD;
    constexpr bool SWAP = !WGRAD;      // D = C^T: lanes along m, the contiguous axis of the forward and input-gradient outputs
    const int lane = thread & 63, wave = thread >> 6;
    const int r = lane & 15, q = lane >> 4;
    // hoisted out of the K loop: the position of the lane's two rows, the (ci, tap) of its two weight-gradient columns
    RtnPos row[2];
    int ci[2], tap[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int m = m0 + 16 * t + r, n = n0 + 16 * t + r;
      row[t] = (WGRAD || m >= p.M) ? RtnPos{0, 0, 0, 0} : rtn_row<MODE>(p, m);
      ci[t] = WGRAD ? rtn_div(n, p.by_taps) : 0;
      tap[t] = WGRAD ? n - ci[t] * p.taps : 0;
    }
    const int hw = p.H * p.W;
    // the lane's operands of the group at k: a[c][t] = A[m0 + 16 t + r][k + 4 c + q], b[c][u] = B[k + 4 c + q][n0 + 16 u + r]
    auto gather = [&](int k, float (&a)[4][2], float (&b)[4][2]) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kc = k + 4 * c + q;
        const bool live = kc < k1;
        if (WGRAD) {
          const RtnPos at = rtn_pos(kc, p.H, p.W);      // once per k, for both rows and both columns
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int m = m0 + 16 * t + r, n = n0 + 16 * t + r;
            a[c][t] = (live && m < p.M) ? p.g[((int64_t)at.bb * p.cout + m) * hw + at.rem] : 0.f;      // rtn_a<RTN_WGRAD>, the position given
            b[c][t] = (live && n < p.N) ? rtn_im2col(p, at, ci[t], tap[t]) : 0.f;
          }
        } else {
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            a[c][t] = live ? rtn_a<MODE>(p, m0 + 16 * t + r, kc, row[t]) : 0.f;
            b[c][t] = live ? rtn_b<MODE>(p, kc, n0 + 16 * t + r) : 0.f;
          }
        }
      }
    };
    const rtn_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    rtn_f32x4 acc[2][2][4];      // [t][u][chain] with SWAP = false, [u][t][chain] with SWAP = true: D's rows first
    double wide[2][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[t][u][c] = zero; wide[t][u][c] = 0.0; }

    float a[4][2], b[4][2], na[4][2], nb[4][2];
    int k = k0 + RTK_GROUP * wave;
    if (k < k1) gather(k, a, b);
    for (; k < k1; k += RTK_GROUP * RTK_WAVES) {      // (wave-uniform)
      const bool more = k + RTK_GROUP * RTK_WAVES < k1;
      if (more) gather(k + RTK_GROUP * RTK_WAVES, na, nb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[t][u][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(SWAP ? b[c][t] : a[c][t], SWAP ? a[c][u] : b[c][u], WIDE ? zero : acc[t][u][c], 0, 0, 0);
          if (WIDE) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
              for (int i = 0; i < 4; ++i) wide[t][u][i] += (double)acc[t][u][c][i];
          }
        }
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int t = 0; t < 2; ++t) { a[c][t] = na[c][t]; b[c][t] = nb[c][t]; }
      }
    }
    // the wave's partial, fragment-major: slot (2 t + u) 4 + i holds accumulator register i of MFMA tile (t, u), 64 lanes each
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const rtn_f32x4 joined = (acc[t][u][0] + acc[t][u][1]) + (acc[t][u][2] + acc[t][u][3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[wave][((2 * t + u) * 4 + i) * 64 + lane] = WIDE ? (S)wide[t][u][i] : (S)joined[i];
      }
    __syncthreads();
    // thread T: MFMA tile (t, u) = T >> 6 at its own lane position, the four accumulator registers, over the waves in a fixed order
    const int t = wave >> 1, u = wave & 1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int at = (wave * 4 + i) * 64 + lane;
      const S sum = (lds[0][at] + lds[1][at]) + (lds[2][at] + lds[3][at]);
      const int x = 16 * t + 4 * q + i, y = 16 * u + r;      // D[x][y]
      rtn_store<MODE>(p, m0 + (SWAP ? y : x), n0 + (SWAP ? x : y), chunk, (float)sum);
    }
#endif
  }
};

#ifdef MZX_TRAIN_GEMM_KSPLIT_DEFINE
#define MZX_KSPLIT_LINKAGE
#else
#define MZX_KSPLIT_LINKAGE inline
#endif

#if defined(MZX_HOSTCHECK) || defined(MZX_TRAIN_GEMM_KSPLIT_DEFINE)
// (declared in mzx_train_resnet.h; the device build compiles it once, in mzx_train_gemm_ksplit.hip)
MZX_KSPLIT_LINKAGE int rtn_launch_ksplit(int mode, bool wide, const RtnGemm& g, stream_t stream) {
  switch (mode * 2 + (wide ? 1 : 0)) {
    case RTN_FWD * 2: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_FWD, false>{g}, stream);
    case RTN_FWD * 2 + 1: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_FWD, true>{g}, stream);
    case RTN_DGRAD * 2: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_DGRAD, false>{g}, stream);
    case RTN_DGRAD * 2 + 1: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_DGRAD, true>{g}, stream);
    case RTN_WGRAD * 2: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_WGRAD, false>{g}, stream);
    default: return launch_tiles<RTK_THREADS>(RtnKsplitGemmBody<RTN_WGRAD, true>{g}, stream);
  }
}
#endif
#undef MZX_KSPLIT_LINKAGE

}  // namespace mzx
