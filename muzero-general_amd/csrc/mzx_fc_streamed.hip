// mzx_fc_streamed.hip -- kernels and launch of the streamed engine for fully connected networks (design and plan:
// mzx_fc_streamed.h): fcs_recurrent_kernel<TM> / fcs_initial_kernel<TM>, TM in {16, 32, 64}, a whole inference per launch.
#include <hip/hip_runtime.h>

#include "mzx_fc_streamed.h"
#include "mzx_wave.h"          // lane_xor: the butterflies of the 16-lane row reductions

namespace mzx {

namespace {

typedef float fcs_f4 __attribute__((ext_vector_type(4)));

struct FcsArgs {
  const float* flat;
  const float* in;           // recurrent: hidden states [batch][in_nodes][E]; initial: observations [batch][in_size]
  const int32_t* action;     // recurrent: [batch]
  const int32_t* in_node;    // null: node 0
  const int32_t* out_node;   // null: node 0
  float* hidden;             // [batch][out_nodes][E]
  float* value;              // [batch][F]
  float* reward;             // [batch][F] (initial: the constant row; may be null there)
  float* policy;             // [batch][A]
  int32_t in_nodes, out_nodes, batch, E, A, F, in_size, in_vec;
  int32_t S, SE, KT;         // LDS row strides (floats) of the ping-pong buffers and of the state buffer; column tiles of a partial
  FcsMlp m[4];               // recurrent: dynamics, reward, policy, value; initial: representation, policy, value
};

// columns per pass of a wave on the column-split route: TM / 16 x FCS_NB accumulator tiles, independent MFMA chains
template <int TM> struct FcsShape { static constexpr int MT = TM / 16, NB = TM == 64 ? 2 : 4; };

// four consecutive k of a global row; beyond K zeros (never dereferenced)
__device__ __forceinline__ fcs_f4 fcs_load4(const float* row, int k, int K, bool vec) {
  if (vec && k + 4 <= K) return *reinterpret_cast<const fcs_f4*>(row + k);
  fcs_f4 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = (k + j < K) ? row[k + j] : 0.f;
  return v;
}

// What a layer reads and writes: x rows in LDS (stride xs) or, XG, in global memory (the observation); y rows in LDS (null:
// none), g rows of an output tensor [batch][N] (null: none).
struct FcsIo {
  const float* x; int xs;
  float* y; int ys;
  float* g;
};

// LinearOp's epilogue on the four consecutive columns n .. n + 3 of tile row r that a lane holds
__device__ __forceinline__ void fcs_epilogue(const FcsArgs& a, const FcsLayer& L, const FcsIo& io, fcs_f4 v, int r, int n, int row0) {
  const float* W = a.flat + L.w;
  const float* bias = a.flat + L.b;
  const int gm = row0 + r;
  const int act = L.onehot ? a.action[gm < a.batch ? gm : a.batch - 1] : 0;
  fcs_f4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int nn = n + c;
    float t = 0.f;
    if (nn < L.N) {
      t = v[c];
      if (L.onehot) t += W[(int64_t)nn * L.w_stride + L.K + act];
      t += bias[nn];
      if (L.elu) t = mzx_elu(t);
    }
    o[c] = t;
  }
  if (io.y) *reinterpret_cast<fcs_f4*>(io.y + r * io.ys + n) = o;
  if (io.g && gm < a.batch) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (n + c < L.N) io.g[(int64_t)gm * L.N + n + c] = o[c];
  }
}

// the lane's X operands of the group at k: rows 16 t + r of the tile
template <int TM, bool XG>
__device__ __forceinline__ void fcs_read_x(const FcsArgs& a, const FcsLayer& L, const FcsIo& io, int r, int k, int row0,
                                           fcs_f4 (&xa)[TM / 16]) {
#pragma unroll
  for (int t = 0; t < TM / 16; ++t) {
    if (XG) {
      const int gm = row0 + 16 * t + r;
      xa[t] = fcs_load4(io.x + (int64_t)(gm < a.batch ? gm : a.batch - 1) * a.in_size, k, L.K, a.in_vec != 0);
    } else {
      xa[t] = *reinterpret_cast<const fcs_f4*>(io.x + (16 * t + r) * io.xs + k);
    }
  }
}

// N >= 64: column tile t to wave t & 3, NB tiles per pass
template <int TM, bool XG>
__device__ __forceinline__ void fcs_layer_nsplit(const FcsArgs& a, const FcsLayer& L, const FcsIo& io, int row0) {
  constexpr int MT = FcsShape<TM>::MT, NB = FcsShape<TM>::NB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int NT = (L.N + 15) / 16, groups = (L.K + 15) / 16;
  const float* W = a.flat + L.w;
  const bool vec = L.vec != 0;
  for (int t0 = wave; t0 < NT; t0 += 4 * NB) {      // (wave-uniform)
    const int live = min(NB, (NT - t0 + 3) / 4);
    const float* wrow[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) wrow[i] = W + (int64_t)min(16 * (t0 + 4 * i) + r, L.N - 1) * L.w_stride;
    fcs_f4 acc[MT][NB], wb[NB], wn[NB], xa[MT];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      wb[i] = i < live ? fcs_load4(wrow[i], 4 * q, L.K, vec) : fcs_f4{0.f, 0.f, 0.f, 0.f};
      wn[i] = fcs_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < MT; ++t) acc[t][i] = fcs_f4{0.f, 0.f, 0.f, 0.f};
    }
    for (int g = 0; g < groups; ++g) {
      const int k = 16 * g + 4 * q;
      const bool more = g + 1 < groups;
      if (more) {
#pragma unroll
        for (int i = 0; i < NB; ++i)
          if (i < live) wn[i] = fcs_load4(wrow[i], k + 16, L.K, vec);
      }
      fcs_read_x<TM, XG>(a, L, io, r, k, row0, xa);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NB; ++i)
        if (i < live) {
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[i][j], xa[t][j], acc[t][i], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
      if (more) {
#pragma unroll
        for (int i = 0; i < NB; ++i) wb[i] = wn[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (i < live) {
#pragma unroll
        for (int t = 0; t < MT; ++t) fcs_epilogue(a, L, io, acc[t][i], 16 * t + r, 16 * (t0 + 4 * i) + 4 * q, row0);
      }
  }
}

// N < 64: group g to wave g & 3, every wave owns all (at most four) column tiles; the partials meet in `part`
template <int TM, bool XG>
__device__ __forceinline__ void fcs_layer_ksplit(const FcsArgs& a, const FcsLayer& L, const FcsIo& io, int row0, float* part) {
  constexpr int MT = FcsShape<TM>::MT, NB = 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int NT = (L.N + 15) / 16, groups = (L.K + 15) / 16;      // NT <= min(NB, a.KT)
  const float* W = a.flat + L.w;
  const bool vec = L.vec != 0;
  const float* wrow[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) wrow[i] = W + (int64_t)min(16 * i + r, L.N - 1) * L.w_stride;
  fcs_f4 acc[MT][NB], wb[NB], wn[NB], xa[MT];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    wb[i] = (i < NT && wave < groups) ? fcs_load4(wrow[i], 16 * wave + 4 * q, L.K, vec) : fcs_f4{0.f, 0.f, 0.f, 0.f};
    wn[i] = fcs_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t][i] = fcs_f4{0.f, 0.f, 0.f, 0.f};
  }
  for (int g = wave; g < groups; g += 4) {      // (wave-uniform)
    const int k = 16 * g + 4 * q;
    const bool more = g + 4 < groups;
    if (more) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
        if (i < NT) wn[i] = fcs_load4(wrow[i], k + 64, L.K, vec);
    }
    fcs_read_x<TM, XG>(a, L, io, r, k, row0, xa);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (i < NT) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[i][j], xa[t][j], acc[t][i], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
    if (more) {
#pragma unroll
      for (int i = 0; i < NB; ++i) wb[i] = wn[i];
    }
  }
  // fragment-major partials [wave][row tile][column tile][register][lane]: 64 consecutive words per store.  A wave without a
  // group writes its zeros all the same: the join never depends on the shape, and nothing relies on cleared LDS.
  const int per_wave = MT * a.KT * 256;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < NB; ++i)
      if (i < NT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) part[wave * per_wave + ((t * a.KT + i) * 4 + c) * 64 + lane] = acc[t][i][c];
      }
  __syncthreads();
  for (int tile = wave; tile < MT * NT; tile += 4) {
    const int t = tile / NT, i = tile - t * NT;
    fcs_f4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float* p = part + ((t * a.KT + i) * 4 + c) * 64 + lane;
      v[c] = (p[0] + p[per_wave]) + (p[2 * per_wave] + p[3 * per_wave]);
    }
    fcs_epilogue(a, L, io, v, 16 * t + r, 16 * i + 4 * q, row0);
  }
}

struct FcsLds { float* buf0; float* buf1; float* state; float* part; };

// One layer on its route, and the barrier behind it
template <int TM, bool XG>
__device__ __forceinline__ void fcs_layer(const FcsArgs& a, const FcsLayer& L, const FcsIo& io, int row0, float* part) {
  if (L.N < FCS_KSPLIT_BELOW) fcs_layer_ksplit<TM, XG>(a, L, io, row0, part);
  else fcs_layer_nsplit<TM, XG>(a, L, io, row0);
  __syncthreads();
}

// Layers first .. of an MLP: x (LDS rows of stride xs) through the ping-pong buffers; the last layer writes LDS rows `last_y`
// (stride last_ys) and / or the output tensor `last_g`.
template <int TM>
__device__ __forceinline__ void fcs_mlp(const FcsArgs& a, const FcsMlp& M, int first, const FcsLds& lds, const float* x, int xs,
                                        float* last_y, int last_ys, float* last_g, int row0) {
  FcsIo io;
  io.x = x; io.xs = xs;
  for (int l = first; l < M.n; ++l) {
    const bool last = l + 1 == M.n;
    io.y = last ? last_y : (io.x == lds.buf0 ? lds.buf1 : lds.buf0);
    io.ys = last ? last_ys : a.S;
    io.g = last ? last_g : nullptr;
    fcs_layer<TM, false>(a, M.l[l], io, row0, lds.part);
    io.x = io.y; io.xs = io.ys;
  }
}

template <int TM>
__device__ __forceinline__ FcsLds fcs_carve(const FcsArgs& a, float* lds) {
  FcsLds o;
  o.buf0 = lds;
  o.buf1 = o.buf0 + TM * a.S;
  o.state = o.buf1 + TM * a.S;
  o.part = o.state + TM * a.SE;
  return o;
}

// MinMaxScaleOp over the E values of every row of the state buffer, in place (s -> h), by a 16-lane row per tree; h also goes
// to the row's node of the hidden-state store.  A barrier behind it.
template <int TM>
__device__ __forceinline__ void fcs_scale(const FcsArgs& a, float* state, int row0) {
  const int sub = threadIdx.x & 15;
  for (int r = threadIdx.x >> 4; r < TM; r += FCS_THREADS / 16) {      // (uniform per 16-lane row: whole rows stay active)
    float* row = state + r * a.SE;
    float lo = MZX_INF, hi = -MZX_INF;
    for (int c = sub; c < a.E; c += 16) { lo = fminf(lo, row[c]); hi = fmaxf(hi, row[c]); }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) { lo = fminf(lo, lane_xor(lo, o)); hi = fmaxf(hi, lane_xor(hi, o)); }      // (xor below 16 stays in the row)
    float scale = hi - lo;
    if (scale < 1e-5f) scale += 1e-5f;
    const int gm = row0 + r;
    const int gc = gm < a.batch ? gm : a.batch - 1;
    const int node = a.out_node ? a.out_node[gc] : 0;
    float* dst = a.hidden + ((int64_t)gc * a.out_nodes + node) * a.E;
    for (int c = sub; c < a.E; c += 16) {
      const float y = mzx_div(row[c] - lo, scale);
      row[c] = y;
      if (gm < a.batch) dst[c] = y;
    }
  }
  __syncthreads();
}

template <int TM>
__global__ void __launch_bounds__(FCS_THREADS) fcs_recurrent_kernel(const FcsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fcs_lds[];
  const FcsLds lds = fcs_carve<TM>(a, fcs_lds);
  const int row0 = blockIdx.x * TM;
  // h_parent of the tile's rows into buffer 0; columns E .. 16-multiple are zero-fed k.  Rows beyond the batch repeat the last.
  const int sub = threadIdx.x & 15, EP = (a.E + 15) & ~15;
  for (int r = threadIdx.x >> 4; r < TM; r += FCS_THREADS / 16) {
    const int gm = row0 + r < a.batch ? row0 + r : a.batch - 1;
    const int node = a.in_node ? a.in_node[gm] : 0;
    const float* src = a.in + ((int64_t)gm * a.in_nodes + node) * a.E;
    for (int c = sub; c < EP; c += 16) lds.buf0[r * a.S + c] = c < a.E ? src[c] : 0.f;
  }
  __syncthreads();
  fcs_mlp<TM>(a, a.m[0], 0, lds, lds.buf0, a.S, lds.state, a.SE, nullptr, row0);      // dynamics: s
  fcs_mlp<TM>(a, a.m[1], 0, lds, lds.state, a.SE, nullptr, 0, a.reward, row0);        // reward on the UNscaled s
  fcs_scale<TM>(a, lds.state, row0);                                                      // h, scattered to the leaf
  fcs_mlp<TM>(a, a.m[2], 0, lds, lds.state, a.SE, nullptr, 0, a.policy, row0);
  fcs_mlp<TM>(a, a.m[3], 0, lds, lds.state, a.SE, nullptr, 0, a.value, row0);
}

template <int TM>
__global__ void __launch_bounds__(FCS_THREADS) fcs_initial_kernel(const FcsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fcs_lds[];
  const FcsLds lds = fcs_carve<TM>(a, fcs_lds);
  const int row0 = blockIdx.x * TM;
  if (a.reward) {      // log of the one-hot at the support's centre (RewardFillOp)
    for (int i = threadIdx.x; i < TM * a.F; i += FCS_THREADS) {
      const int r = i / a.F, c = i - r * a.F;
      if (row0 + r < a.batch) a.reward[(int64_t)(row0 + r) * a.F + c] = (c == a.F / 2) ? 0.0f : -(float)MZX_INF;
    }
  }
  // representation: its first layer reads the observation from global memory, the rest runs from buffer 0
  const bool one = a.m[0].n == 1;
  const FcsIo first = {a.in, 0, one ? lds.state : lds.buf0, one ? a.SE : a.S, nullptr};
  fcs_layer<TM, true>(a, a.m[0].l[0], first, row0, lds.part);
  fcs_mlp<TM>(a, a.m[0], 1, lds, lds.buf0, a.S, lds.state, a.SE, nullptr, row0);
  fcs_scale<TM>(a, lds.state, row0);
  fcs_mlp<TM>(a, a.m[1], 0, lds, lds.state, a.SE, nullptr, 0, a.policy, row0);
  fcs_mlp<TM>(a, a.m[2], 0, lds, lds.state, a.SE, nullptr, 0, a.value, row0);
}

template <int TM>
int fcs_launch(bool recurrent, const FcsArgs& a, int lds_bytes, stream_t stream) {
  static std::atomic<uint64_t> done[2];
  const void* fn = recurrent ? (const void*)&fcs_recurrent_kernel<TM> : (const void*)&fcs_initial_kernel<TM>;
  if (lds_bytes > 64 * 1024) {
    const int e = allow_large_lds(fn, FCS_LDS_BUDGET, done[recurrent ? 1 : 0]);
    if (e) return e;
  }
  const dim3 grid((unsigned)((a.batch + TM - 1) / TM)), block(FCS_THREADS);
  if (recurrent) hipLaunchKernelGGL(fcs_recurrent_kernel<TM>, grid, block, lds_bytes, stream, a);
  else hipLaunchKernelGGL(fcs_initial_kernel<TM>, grid, block, lds_bytes, stream, a);
  return (int)hipGetLastError();
}

}  // namespace

int fcs_run(const mzx_net* net, bool recurrent, const NetBuffers& nb, int batch, stream_t stream, const NetIndex* ix) {
  const FcsPlan& P = net->fcs;      // (kept by mzx_net_set_fc_engine)
  if (!P.ok) { set_error("fully connected streamed engine: the handle has no plan (mzx_net_set_fc_engine)"); return MZX_ERR_INVALID; }
  const int TM = fcs_choose_tm(P, recurrent, batch, tune(TUNE_FCS_TM));
  if (!TM) { set_error("fully connected streamed engine: activations beyond 160 KiB of LDS"); return MZX_ERR_INVALID; }
  if (recurrent && !nb.action) { set_error("fully connected streamed engine: recurrent inference needs actions"); return MZX_ERR_INVALID; }
  FcsArgs a;
  memset(&a, 0, sizeof(a));
  a.flat = net->d_flat; a.in = nb.in; a.action = nb.action;
  a.in_node = ix ? ix->in_node : nullptr; a.out_node = ix ? ix->out_node : nullptr;
  a.in_nodes = ix ? ix->in_nodes : 1; a.out_nodes = ix ? ix->out_nodes : 1;
  a.hidden = nb.hidden; a.value = nb.value; a.reward = nb.reward; a.policy = nb.policy;
  a.batch = batch; a.E = P.E; a.A = P.A; a.F = P.F; a.in_size = P.in_size;
  a.in_vec = (P.in_size % 4 == 0 && ((uintptr_t)nb.in & 15) == 0) ? 1 : 0;
  const int w = recurrent ? 1 : 0;
  a.S = fcs_stride(P.width[w]); a.SE = fcs_stride(P.E); a.KT = P.ks_tiles[w];
  if (recurrent) { a.m[0] = P.dyn; a.m[1] = P.rew; a.m[2] = P.pol; a.m[3] = P.val; }
  else { a.m[0] = P.rep; a.m[1] = P.pol; a.m[2] = P.val; }
  if ((uintptr_t)net->d_flat & 15)      // (128-bit weight loads need the flat buffer on a 16-byte boundary)
    for (FcsMlp& m : a.m)
      for (FcsLayer& l : m.l) l.vec = 0;
  const int lds = (int)fcs_lds_bytes(P, recurrent, TM);
  const int rc = TM == 64 ? fcs_launch<64>(recurrent, a, lds, stream) : TM == 32 ? fcs_launch<32>(recurrent, a, lds, stream)
                                                                               : fcs_launch<16>(recurrent, a, lds, stream);
  if (rc) { set_error("kernel launch failed: %s", runtime_error_string(rc)); return MZX_ERR_RUNTIME; }
  return MZX_OK;
}

}  // namespace mzx
