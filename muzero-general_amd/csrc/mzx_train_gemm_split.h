// mzx_train_gemm_split.h -- the second ARITHMETIC of the residual trainer's LDS-tiled GEMM route (mzx_train_gemm_tiled.h):
// RtnSplitGemmBody<MODE, WIDE>, the same 256-thread workgroup per (weight-gradient chunk, 64 x 64 output tile) and the same
// RtnGemm descriptor and operand functions (rtn_row / rtn_a / rtn_b / rtn_im2col / rtn_pos / rtn_store<MODE>), but the
// products run on the BF16 matrix pipes (v_mfma_f32_16x16x32_bf16) with every binary32 operand split into three BF16 terms.
// A GEMM that the handle's train_gemm switch sends to the tiled route takes this body when the handle's train_matrix switch
// (mzx_net_set_train_matrix) is MZX_TRAIN_MATRIX_BF16X3, and RtnTileGemmBody otherwise.  Its contract is the reference
// gates of the training tests, NOT the bits of the wave body.
//
// The arithmetic.  Under round-to-nearest-even a binary32 x is exactly h + m + l with
//     h = bf16(x)      m = bf16(x - h)      l = bf16(x - h - m)            |m| <= 2^-8 |x|,  |l| <= 2^-16 |x|
// (both subtractions are exact in binary32: each remainder has no more significant bits than x has left; the build keeps
// -ffp-contract=off).  A BF16 x BF16 product is exact in binary32, and the MFMA accumulates in binary32.  Of the nine partial
// products of a x b six are issued, per 16 x 16 output tile and slab of 32 k in this fixed order, smallest first:
//     l.h   h.l   m.m   m.h   h.m   h.h                                    (written A-term . B-term)
// The three dropped ones, m.l + l.m + l.l, are below 2^-23 |a| |b| (2^-24 + 2^-24 + 2^-32): under the rounding of ONE binary32
// addition, and about ninety times below what binary32 accumulation over a K of a few thousand leaves anyway.  Three
// products (h.h, h.m, m.h) would leave 2^-16 |a| |b| per term and do not hold the trainer's gates.
// WIDE = false: ONE accumulator chain per output tile, carried through the 6 MFMAs of every slab of the chunk; a wave
// issues a product for its four tiles before the next product, so dependent MFMAs are four apart.
// WIDE = true (networks with a downsample stem): every MFMA starts from zero and its result is added, in issue order, to the
// tile's binary64 accumulators, rounded once at the end: the WIDE contract of the other bodies with 32 k per join.
// No atomics; chunks, RtnWgradFinishOp and every epilogue are those of the other bodies: a second call reproduces every bit.
//
// Work split.  Four waves as 2 x 2: wave (wm, wn) owns the 32 x 32 quadrant at (32 wm, 32 wn), four 16 x 16 MFMA tiles (t, u):
// the routing rule of mzx_tuning.h means what it means for RtnTileGemmBody.  For v_mfma_f32_16x16x32_bf16 lane l feeds
// A[l & 15][8 (l >> 4) .. + 7] and B[8 (l >> 4) .. + 7][l & 15] -- eight consecutive k of one row / column -- and holds
// D[4 (l >> 4) + i][l & 15] in accumulator register i, as for 16x16x4.  Per slab a wave makes 12 fragment reads (2 row tiles
// and 2 column tiles x 3 planes) and 24 MFMAs (4 tiles x 6 products), where the binary32 body issues 32 of a quarter the k.
//
// Data movement.  K is walked in slabs of 32, one MFMA k-extent.  Per slab the workgroup gathers A [64][32] and B [64][32] once,
// 8 + 8 binary32 elements per thread along the operand's contiguous global axis, zero beyond M, N and the chunk's end:
//     position-fast (A forward / input gradient, B input gradient)   row = thread & 63, k = 8 (thread >> 6) + i
//     k-fast (A / B weight gradient, B forward)                      k = thread & 31, row = (thread >> 5) + 8 i
// (row: the operand's row of A or column of B inside the tile).  The position of a thread's row, the position of a
// weight-gradient k (once per slab) and the (ci, tap) of a weight-gradient column are hoisted as in RtnTileGemmBody.  The
// loads of slab s + 1 are issued before the MFMAs of slab s.
// The split happens at staging: each gathered element is split ONCE per workgroup, in registers (v_cvt_pk_bf16_f32 is RNE),
// and its three terms go to three BF16 planes, so the conversions are paid per element, not per wave or per MFMA.
//
// LDS: [buffer 2][A | B][plane h, m, l][row 64][chunk 4] of 16-byte chunks (eight BF16 = eight consecutive k), 48 KB static,
// no padding: row `row` keeps its k-chunk c at chunk index c ^ ((row >> 2) & 3).  Banks (64 of 4 bytes; a 16-byte access is
// served per group of 16 lanes): a chunk starts at dword 16 row + 4 (c ^ ((row >> 2) & 3)), i.e. bank 16 (row & 3) +
// 4 (c ^ ((row >> 2) & 3)) (mod 64).
//   * Fragment read (ds_read_b128): the 16 lanes of a group share c = l >> 4 and read rows base + 0 .. 15 (base a multiple of
//     16): row & 3 and (row >> 2) & 3 take all 16 combinations, so the 16 chunks start at the 16 different multiples of four:
//     all 64 banks once, conflict-free.
//   * Position-fast writers hold the eight k of one chunk of one row: one ds_write_b128 per plane, 64 consecutive rows per
//     wave at one c -- the read pattern, conflict-free.
//   * k-fast writers store 2-byte elements: a wave covers the 32 k of two consecutive rows (an even row and the next): the
//     XOR permutes the four chunks inside a row's 16 dwords and the two rows lie 16 dwords apart: 32 different dwords, two
//     lanes per dword, nothing serialised.
// Two buffers; the next slab is written to the other buffer behind this slab's MFMAs; one barrier per slab.  Every element
// of a buffer is written before it is read (a ragged slab stages zeros): nothing relies on zeroed LDS.
//
// tests/hostcheck build: rts_serial_tile, a plain restatement of the definition above over the 64 x 64 tile: operands split by
// an integer-exact RNE helper, per slab the six products summed over increasing k in the order above into a binary32
// accumulator (from zero each, joined in binary64, under WIDE).  The MFMA's internal summation order is the hardware's, so
// the two builds do not agree bit for bit; both are held to the same gates.
#pragma once
#include "mzx_train_resnet.h"

namespace mzx {

constexpr int RTS_THREADS = 256;
constexpr int RTS_TILE = 64;         // rows and columns of a workgroup's output tile
constexpr int RTS_SLAB = 32;         // k per LDS buffer: one v_mfma_f32_16x16x32_bf16
constexpr int RTS_PER_THREAD = RTS_SLAB * RTS_TILE / RTS_THREADS;      // elements of one operand's slab a thread gathers
constexpr int RTS_PRODUCTS = 6;
// the planes (0 h, 1 m, 2 l) of A and of B in product p: l.h, h.l, m.m, m.h, h.m, h.h
#define RTS_PLANE_A(p) ((p) == 0 ? 2 : ((p) == 2 || (p) == 3) ? 1 : 0)
#define RTS_PLANE_B(p) ((p) == 1 ? 2 : ((p) == 2 || (p) == 4) ? 1 : 0)

#ifdef MZX_HOSTCHECK
// binary32 -> the nearest BF16 (ties to even), returned as the binary32 of the same value
inline float rts_bf16_rne(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  u += 0x7fffu + ((u >> 16) & 1u);
  u &= 0xffff0000u;
  memcpy(&x, &u, 4);
  return x;
}
inline void rts_split(float x, float* out) {
  out[0] = rts_bf16_rne(x);
  const float r = x - out[0];
  out[1] = rts_bf16_rne(r);
  out[2] = rts_bf16_rne(r - out[1]);
}
template <int MODE, bool WIDE>
inline void rts_serial_tile(const RtnGemm& p, int m0, int n0, int chunk, int k0, int k1) {
  for (int i = 0; i < RTS_TILE; ++i) {
    const int m = m0 + i;
    if (m >= p.M) break;
    const RtnPos row = rtn_row<MODE>(p, m);
    for (int j = 0; j < RTS_TILE; ++j) {
      const int n = n0 + j;
      if (n >= p.N) break;
      float acc = 0.f;
      double wide = 0.0;
      for (int ks = k0; ks < k1; ks += RTS_SLAB) {
        float a[RTS_SLAB][3], b[RTS_SLAB][3];
        for (int kk = 0; kk < RTS_SLAB; ++kk) {
          const int k = ks + kk;
          rts_split(k < k1 ? rtn_a<MODE>(p, m, k, row) : 0.f, a[kk]);
          rts_split(k < k1 ? rtn_b<MODE>(p, k, n) : 0.f, b[kk]);
        }
        for (int pr = 0; pr < RTS_PRODUCTS; ++pr) {
          float t = 0.f;
          float& sum = WIDE ? t : acc;
          for (int kk = 0; kk < RTS_SLAB; ++kk) sum += a[kk][RTS_PLANE_A(pr)] * b[kk][RTS_PLANE_B(pr)];
          if (WIDE) wide += (double)t;
        }
      }
      rtn_store<MODE>(p, m, n, chunk, WIDE ? (float)wide : acc);
    }
  }
}
#else
typedef __bf16 rts_bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t rts_u32x4 __attribute__((ext_vector_type(4)));
#endif

template <int MODE, bool WIDE>
struct RtnSplitGemmBody {
  RtnGemm p;
  MZX_HD int tiles_n() const { return (p.N + RTS_TILE - 1) / RTS_TILE; }
  MZX_HD size_t size() const { return (size_t)((p.M + RTS_TILE - 1) / RTS_TILE) * tiles_n() * p.nchunks; }
  MZX_WAVE_FN void operator()(size_t item, int thread) const {
    const int tiles = ((p.M + RTS_TILE - 1) / RTS_TILE) * tiles_n();
    const int chunk = (int)(item / tiles), tile = (int)(item % tiles);
    const int m0 = (tile / tiles_n()) * RTS_TILE, n0 = (tile % tiles_n()) * RTS_TILE;
    const int k0 = chunk * p.kchunk;
    const int k1 = (p.K - k0 < p.kchunk) ? p.K : k0 + p.kchunk;
#ifdef MZX_HOSTCHECK
    (void)thread;
    rts_serial_tile<MODE, WIDE>(p, m0, n0, chunk, k0, k1);
#else
    __shared__ rts_u32x4 lds[2][2][3][RTS_TILE * 4];      // [buffer][A | B][plane][row * 4 + (chunk ^ ((row >> 2) & 3))]
    constexpr bool A_KFAST = MODE == RTN_WGRAD, B_KFAST = MODE != RTN_DGRAD;
    const int lane = thread & 63, wave = thread >> 6;
    const int r = lane & 15, q = lane >> 4, wm = wave >> 1, wn = wave & 1;
    // what a thread gathers: element i of its A and of its B, as (k, row) inside the slab
    const int ka = A_KFAST ? (thread & 31) : 8 * (thread >> 6), ca = A_KFAST ? (thread >> 5) : (thread & 63);
    const int kb = B_KFAST ? (thread & 31) : 8 * (thread >> 6), cb = B_KFAST ? (thread >> 5) : (thread & 63);
    constexpr int KA_STEP = A_KFAST ? 0 : 1, CA_STEP = A_KFAST ? 8 : 0, KB_STEP = B_KFAST ? 0 : 1, CB_STEP = B_KFAST ? 8 : 0;
    // hoisted out of the K loop: the position of the thread's row, the (ci, tap) of its weight-gradient columns
    const RtnPos row = (A_KFAST || m0 + ca >= p.M) ? RtnPos{0, 0, 0, 0} : rtn_row<MODE>(p, m0 + ca);
    int ci[RTS_PER_THREAD], tap[RTS_PER_THREAD];
    if (MODE == RTN_WGRAD) {
#pragma unroll
      for (int i = 0; i < RTS_PER_THREAD; ++i) {
        const int n = n0 + cb + CB_STEP * i;
        ci[i] = rtn_div(n, p.by_taps);
        tap[i] = n - ci[i] * p.taps;
      }
    }
    float ra[RTS_PER_THREAD], rb[RTS_PER_THREAD];
    auto gather = [&](int ks) {
#pragma unroll
      for (int i = 0; i < RTS_PER_THREAD; ++i) {
        const int k = ks + ka + KA_STEP * i;
        ra[i] = k < k1 ? rtn_a<MODE>(p, m0 + ca + CA_STEP * i, k, row) : 0.f;
      }
      if (MODE == RTN_WGRAD) {
        const int k = ks + kb;
        const RtnPos at = rtn_pos(k, p.H, p.W);
#pragma unroll
        for (int i = 0; i < RTS_PER_THREAD; ++i)
          rb[i] = (k < k1 && n0 + cb + CB_STEP * i < p.N) ? rtn_im2col(p, at, ci[i], tap[i]) : 0.f;
      } else {
#pragma unroll
        for (int i = 0; i < RTS_PER_THREAD; ++i) {
          const int k = ks + kb + KB_STEP * i;
          rb[i] = k < k1 ? rtn_b<MODE>(p, k, n0 + cb + CB_STEP * i) : 0.f;
        }
      }
    };
    // split a thread's eight elements of one operand and write the three planes
    auto stage_operand = [&](rts_u32x4 (*planes)[RTS_TILE * 4], const float* v, bool kfast, int k, int c, int cstep) {
      rts_bf16x8 term[3];
#pragma unroll
      for (int i = 0; i < RTS_PER_THREAD; ++i) {
        const __bf16 h = (__bf16)v[i];
        const float rest = v[i] - (float)h;
        const __bf16 m = (__bf16)rest;
        term[0][i] = h; term[1][i] = m; term[2][i] = (__bf16)(rest - (float)m);
      }
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) {
        if (kfast) {      // element i: (k, row c + cstep i), two bytes each
          __bf16* half = reinterpret_cast<__bf16*>(planes[pl]);
#pragma unroll
          for (int i = 0; i < RTS_PER_THREAD; ++i) {
            const int rw = c + cstep * i;
            half[(rw * 4 + ((k >> 3) ^ ((rw >> 2) & 3))) * 8 + (k & 7)] = term[pl][i];
          }
        } else {          // the eight k of chunk k >> 3 of row c
          planes[pl][c * 4 + ((k >> 3) ^ ((c >> 2) & 3))] = __builtin_bit_cast(rts_u32x4, term[pl]);
        }
      }
    };
    auto stage = [&](int buf) {
      stage_operand(lds[buf][0], ra, A_KFAST, ka, ca, CA_STEP);
      stage_operand(lds[buf][1], rb, B_KFAST, kb, cb, CB_STEP);
    };
    const rtn_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    rtn_f32x4 acc[2][2];
    double wide[2][2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        acc[t][u] = zero;
#pragma unroll
        for (int i = 0; i < 4; ++i) wide[t][u][i] = 0.0;
      }
    // a lane's fragment of row tile t: chunk q of row 32 w + 16 t + r, whose (row >> 2) & 3 is r >> 2
    const int frag_a = (32 * wm + r) * 4 + (q ^ (r >> 2)), frag_b = (32 * wn + r) * 4 + (q ^ (r >> 2));

    gather(k0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int ks = k0; ks < k1; ks += RTS_SLAB, buf ^= 1) {
      const bool more = ks + RTS_SLAB < k1;
      if (more) gather(ks + RTS_SLAB);
      rts_bf16x8 a[3][2], b[3][2];
#pragma unroll
      for (int pl = 0; pl < 3; ++pl)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          a[pl][t] = __builtin_bit_cast(rts_bf16x8, lds[buf][0][pl][frag_a + 16 * 4 * t]);
          b[pl][t] = __builtin_bit_cast(rts_bf16x8, lds[buf][1][pl][frag_b + 16 * 4 * t]);
        }
#pragma unroll
      for (int pr = 0; pr < RTS_PRODUCTS; ++pr)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[RTS_PLANE_A(pr)][t], b[RTS_PLANE_B(pr)][u], WIDE ? zero : acc[t][u], 0, 0, 0);
            if (WIDE) {
#pragma unroll
              for (int i = 0; i < 4; ++i) wide[t][u][i] += (double)acc[t][u][i];
            }
          }
      if (more) stage(buf ^ 1);
      __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          rtn_store<MODE>(p, m0 + 32 * wm + 16 * t + 4 * q + i, n0 + 32 * wn + 16 * u + r, chunk, WIDE ? (float)wide[t][u][i] : acc[t][u][i]);
#endif
  }
};

#ifdef MZX_TRAIN_GEMM_SPLIT_DEFINE
#define MZX_SPLIT_LINKAGE
#else
#define MZX_SPLIT_LINKAGE inline
#endif

#if defined(MZX_HOSTCHECK) || defined(MZX_TRAIN_GEMM_SPLIT_DEFINE)
// (declared in mzx_train_resnet.h; the device build compiles it once, in mzx_train_gemm_split.hip)
MZX_SPLIT_LINKAGE int rtn_launch_split(int mode, bool wide, const RtnGemm& g, stream_t stream) {
  switch (mode * 2 + (wide ? 1 : 0)) {
    case RTN_FWD * 2: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_FWD, false>{g}, stream);
    case RTN_FWD * 2 + 1: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_FWD, true>{g}, stream);
    case RTN_DGRAD * 2: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_DGRAD, false>{g}, stream);
    case RTN_DGRAD * 2 + 1: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_DGRAD, true>{g}, stream);
    case RTN_WGRAD * 2: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_WGRAD, false>{g}, stream);
    default: return launch_tiles<RTS_THREADS>(RtnSplitGemmBody<RTN_WGRAD, true>{g}, stream);
  }
}
#endif
#undef MZX_SPLIT_LINKAGE

}  // namespace mzx
