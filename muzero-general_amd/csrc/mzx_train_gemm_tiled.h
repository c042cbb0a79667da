// mzx_train_gemm_tiled.h -- the second GEMM variant of the residual trainer (mzx_train_resnet.h, "The three GEMMs"):
// RtnTileGemmBody<MODE, WIDE>, a 256-thread workgroup per (weight-gradient chunk, 64 x 64 output tile), the operands staged
// through LDS.  It serves the same RtnGemm descriptor through the same operand functions (rtn_a / rtn_b / rtn_im2col /
// rtn_store<MODE>) as RtnGemmBody and returns the same bits; which of the two a GEMM of the step takes is the handle's
// train_gemm switch (mzx_net_set_train_gemm) and the rule of mzx_tuning.h.
//
// Work split.  Four waves as 2 x 2: wave (wm, wn) owns the 32 x 32 quadrant at (32 wm, 32 wn) of the tile, four 16 x 16 MFMA
// tiles (t, u), each with the four accumulator chains of RtnGemmBody (64 accumulator registers; WIDE adds four doubles per
// MFMA tile).  Rows, columns and k beyond M, N and the chunk's end are zero operands -- the operand functions' own returns
// and the `k < k1` test of the wave body -- and rtn_store drops what lies outside: no buffer is read or written past its end.
//
// Data movement.  K is walked in slabs of 32.  Per slab the workgroup gathers A [32][64] and B [32][64] once, 8 + 8 elements
// per thread, instead of once per wave.  A thread's elements lie along the operand's contiguous axis in global memory:
//     A  forward, input gradient   column (position) = thread & 63, k = (thread >> 6) + 4 i      im2col(x) / dz
//     A  weight gradient           k (position) = thread & 31, row = (thread >> 5) + 8 i           dz^T
//     B  forward                   k = thread & 31, column = (thread >> 5) + 8 i                   w[n][k]
//     B  input gradient            column = thread & 63, k = (thread >> 6) + 4 i                   w[co][n][tap]
//     B  weight gradient           k (position) = thread & 31, column = (thread >> 5) + 8 i        im2col(x)
// so the position of a thread's row (rtn_pos) is found once per GEMM, the position of a weight-gradient k once per slab, and
// the (ci, tap) of a weight-gradient column once per GEMM.
// LDS: [buffer][A | B][k][column ^ (k >> 2)] with a row stride of 80 floats (64 + 16).  An MFMA k-quad reads the rows 4 c + q
// (q = lane >> 4) at 16 consecutive columns: 80 q = 16 q (mod 64), four disjoint groups of 16 banks, and the XOR is uniform
// over q, a permutation inside the 16 columns.  A k-fast writer (32 values of k at one column) lands on 4 x 8 different banks
// instead of four.  A k-quad costs a wave four ds_read_b32 for four MFMAs.  Two buffers, 40 KB static: the global loads of
// slab s + 1 are issued into registers before the MFMAs of slab s and written to the other buffer behind them; one barrier
// per slab.  Every element of a buffer is written before it is read: nothing relies on zeroed LDS.
//
// Same bits.  Per output element the body issues the MFMAs of RtnGemmBody with the same operand values in the same
// per-chain order: a slab is two k-groups of 16 that start at the chunk's k0 (a multiple of RTN_KCHUNK = 16 slabs), chain c
// of a group takes k + 4 c .. k + 4 c + 3, a ragged last group is fed zeros, and a group that starts at or beyond the
// chunk's end is not issued at all (an all-zero MFMA would turn a -0.0 accumulator into +0.0).  The join, the binary64
// accumulation of WIDE, the weight-gradient chunks and RtnWgradFinishOp are the wave body's.
//
// tests/hostcheck build: the tile is rtn_serial_tile, the loop RtnGemmBody runs there, over 64 x 64.
#pragma once
#include "mzx_train_resnet.h"

namespace mzx {

constexpr int RTT_THREADS = 256;
constexpr int RTT_TILE = 64;         // rows and columns of a workgroup's output tile
constexpr int RTT_SLAB = 32;         // k per LDS buffer: two MFMA k-groups of 16
constexpr int RTT_STRIDE = 80;       // floats per k row in LDS
constexpr int RTT_PER_THREAD = RTT_SLAB * RTT_TILE / RTT_THREADS;      // elements of one operand's slab a thread gathers

template <int MODE, bool WIDE>
struct RtnTileGemmBody {
  RtnGemm p;
  MZX_HD int tiles_n() const { return (p.N + RTT_TILE - 1) / RTT_TILE; }
  MZX_HD size_t size() const { return (size_t)((p.M + RTT_TILE - 1) / RTT_TILE) * tiles_n() * p.nchunks; }
  MZX_WAVE_FN void operator()(size_t item, int thread) const {
    const int tiles = ((p.M + RTT_TILE - 1) / RTT_TILE) * tiles_n();
    const int chunk = (int)(item / tiles), tile = (int)(item % tiles);
    const int m0 = (tile / tiles_n()) * RTT_TILE, n0 = (tile % tiles_n()) * RTT_TILE;
    const int k0 = chunk * p.kchunk;
    const int k1 = (p.K - k0 < p.kchunk) ? p.K : k0 + p.kchunk;
#ifdef MZX_HOSTCHECK
    (void)thread;
    rtn_serial_tile<MODE, WIDE>(p, m0, n0, RTT_TILE, chunk, k0, k1);
#else
    __shared__ float lds[2][2][RTT_SLAB * RTT_STRIDE];
    constexpr bool A_KFAST = MODE == RTN_WGRAD, B_KFAST = MODE != RTN_DGRAD;
    const int lane = thread & 63, wave = thread >> 6;
    const int r = lane & 15, q = lane >> 4, wm = wave >> 1, wn = wave & 1;
    // what a thread gathers: element i of its A and of its B, as (k, column) inside the slab
    const int ka = A_KFAST ? (thread & 31) : (thread >> 6), ca = A_KFAST ? (thread >> 5) : (thread & 63);
    const int kb = B_KFAST ? (thread & 31) : (thread >> 6), cb = B_KFAST ? (thread >> 5) : (thread & 63);
    constexpr int KA_STEP = A_KFAST ? 0 : 4, CA_STEP = A_KFAST ? 8 : 0, KB_STEP = B_KFAST ? 0 : 4, CB_STEP = B_KFAST ? 8 : 0;
    // hoisted out of the K loop: the position of the thread's row, the (ci, tap) of its weight-gradient columns
    const RtnPos row = (A_KFAST || m0 + ca >= p.M) ? RtnPos{0, 0, 0, 0} : rtn_row<MODE>(p, m0 + ca);
    int ci[RTT_PER_THREAD], tap[RTT_PER_THREAD];
    if (MODE == RTN_WGRAD) {
#pragma unroll
      for (int i = 0; i < RTT_PER_THREAD; ++i) {
        const int n = n0 + cb + CB_STEP * i;
        ci[i] = rtn_div(n, p.by_taps);
        tap[i] = n - ci[i] * p.taps;
      }
    }
    float ra[RTT_PER_THREAD], rb[RTT_PER_THREAD];
    auto gather = [&](int ks) {
#pragma unroll
      for (int i = 0; i < RTT_PER_THREAD; ++i) {
        const int k = ks + ka + KA_STEP * i;
        ra[i] = k < k1 ? rtn_a<MODE>(p, m0 + ca + CA_STEP * i, k, row) : 0.f;
      }
      if (MODE == RTN_WGRAD) {
        const int k = ks + kb;
        const RtnPos at = rtn_pos(k, p.H, p.W);
#pragma unroll
        for (int i = 0; i < RTT_PER_THREAD; ++i)
          rb[i] = (k < k1 && n0 + cb + CB_STEP * i < p.N) ? rtn_im2col(p, at, ci[i], tap[i]) : 0.f;
      } else {
#pragma unroll
        for (int i = 0; i < RTT_PER_THREAD; ++i) {
          const int k = ks + kb + KB_STEP * i;
          rb[i] = k < k1 ? rtn_b<MODE>(p, k, n0 + cb + CB_STEP * i) : 0.f;
        }
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int i = 0; i < RTT_PER_THREAD; ++i) {
        const int k = ka + KA_STEP * i, kk = kb + KB_STEP * i;
        lds[buf][0][k * RTT_STRIDE + ((ca + CA_STEP * i) ^ (k >> 2))] = ra[i];
        lds[buf][1][kk * RTT_STRIDE + ((cb + CB_STEP * i) ^ (kk >> 2))] = rb[i];
      }
    };
    const rtn_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    rtn_f32x4 acc[2][2][4];
    double wide[2][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[t][u][c] = zero; wide[t][u][c] = 0.0; }

    gather(k0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int ks = k0; ks < k1; ks += RTT_SLAB, buf ^= 1) {
      const bool more = ks + RTT_SLAB < k1;
      if (more) gather(ks + RTT_SLAB);
      const float* sa = lds[buf][0];
      const float* sb = lds[buf][1];
#pragma unroll
      for (int g = 0; g < RTT_SLAB / 16; ++g) {
        if (ks + 16 * g >= k1) break;      // (workgroup-uniform) a group the wave body does not issue
        float a[4][2], b[4][2];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = 16 * g + 4 * c + q, swz = 4 * g + c;      // swz = k >> 2
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            a[c][t] = sa[k * RTT_STRIDE + ((32 * wm + 16 * t + r) ^ swz)];
            b[c][t] = sb[k * RTT_STRIDE + ((32 * wn + 16 * t + r) ^ swz)];
          }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              acc[t][u][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][t], b[c][u], WIDE ? zero : acc[t][u][c], 0, 0, 0);
            if (WIDE) {
#pragma unroll
              for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) wide[t][u][i] += (double)acc[t][u][c][i];
            }
          }
      }
      if (more) stage(buf ^ 1);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const rtn_f32x4 joined = (acc[t][u][0] + acc[t][u][1]) + (acc[t][u][2] + acc[t][u][3]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          rtn_store<MODE>(p, m0 + 32 * wm + 16 * t + 4 * q + i, n0 + 32 * wn + 16 * u + r, chunk, WIDE ? (float)wide[t][u][i] : joined[i]);
      }
#endif
  }
};

#ifdef MZX_TRAIN_GEMM_TILED_DEFINE
#define MZX_TILED_LINKAGE
#else
#define MZX_TILED_LINKAGE inline
#endif

#if defined(MZX_HOSTCHECK) || defined(MZX_TRAIN_GEMM_TILED_DEFINE)
// (declared in mzx_train_resnet.h; the device build compiles it once, in mzx_train_gemm_tiled.hip)
MZX_TILED_LINKAGE int rtn_launch_tiled(int mode, bool wide, const RtnGemm& g, stream_t stream) {
  switch (mode * 2 + (wide ? 1 : 0)) {
    case RTN_FWD * 2: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_FWD, false>{g}, stream);
    case RTN_FWD * 2 + 1: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_FWD, true>{g}, stream);
    case RTN_DGRAD * 2: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_DGRAD, false>{g}, stream);
    case RTN_DGRAD * 2 + 1: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_DGRAD, true>{g}, stream);
    case RTN_WGRAD * 2: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_WGRAD, false>{g}, stream);
    default: return launch_tiles<RTT_THREADS>(RtnTileGemmBody<RTN_WGRAD, true>{g}, stream);
  }
}
#endif
#undef MZX_TILED_LINKAGE

}  // namespace mzx
