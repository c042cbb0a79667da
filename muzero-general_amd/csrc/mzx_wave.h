// mzx_wave.h -- one body for a wave-cooperative kernel in both builds.
//
// A wave body is written for "my lane of WAVE_LANES": lane-stride loops (WAVE_FOR) followed by cross-lane steps.  Product
// build: WAVE_LANES = 64, the cross-lane steps are the __shfl / __ballot forms, launch_waves (mzx_launch.h) gives every
// work item a wavefront.  tests/hostcheck build: WAVE_LANES = 1 and lane = 0, so a lane-stride loop visits every index in
// increasing order, every butterfly and scan has no levels (the loops over `o` below run zero times) and a broadcast is
// the value itself: the body IS the serial statement, sums taken in increasing index order.
// The block-level analogue for the one-workgroup finishing reductions (launch_block): block_threads(BLOCK) threads, an LDS
// array of that many partials (MZX_BLOCK_SHARED), block_sync() between the levels of the tree -- one thread, no levels,
// the sequential sum in the hostcheck build.
#pragma once
#include "mzx_platform.h"

namespace mzx {

#ifdef MZX_HOSTCHECK
constexpr int WAVE_LANES = 1;
#define MZX_WAVE_FN inline
#define MZX_BLOCK_SHARED
template <class T> inline T lane_xor(T v, int) { return v; }
template <class T> inline T lane_up(T v, int) { return v; }
template <class T> inline T lane_value(T v, int) { return v; }
inline int wave_first_lane(bool flag) { return flag ? 0 : -1; }
inline int wave_last_lane(bool flag) { return flag ? 0 : -1; }
inline uint64_t wave_ballot(bool flag) { return flag ? 1u : 0u; }
inline int wave_rank_below(uint64_t, int) { return 0; }
constexpr int block_threads(int) { return 1; }
inline void block_sync() {}
inline void wave_atomic_add(int32_t* p, int32_t v) { *p += v; }
inline void wave_atomic_or(int32_t* p, int32_t v) { *p |= v; }
inline void wave_fence() {}
#else
constexpr int WAVE_LANES = 64;
#define MZX_WAVE_FN __device__ __forceinline__
#define MZX_BLOCK_SHARED __shared__
template <class T> __device__ __forceinline__ T lane_xor(T v, int o) { return __shfl_xor(v, o, 64); }
template <class T> __device__ __forceinline__ T lane_up(T v, int o) { return __shfl_up(v, o, 64); }      // lanes < o keep v
template <class T> __device__ __forceinline__ T lane_value(T v, int k) { return __shfl(v, k, 64); }      // v of lane k
// the first / last lane whose flag is set (-1: none), the same value in every lane
__device__ __forceinline__ int wave_first_lane(bool flag) {
  const uint64_t set = __ballot(flag);
  return set ? __ffsll((long long)set) - 1 : -1;
}
__device__ __forceinline__ int wave_last_lane(bool flag) {
  const uint64_t set = __ballot(flag);
  return set ? 63 - __clzll((long long)set) : -1;
}
// bit l = lane l's flag, the same value in every lane; how many set bits lie below `lane` (a stable compaction's slot)
__device__ __forceinline__ uint64_t wave_ballot(bool flag) { return __ballot(flag); }
__device__ __forceinline__ int wave_rank_below(uint64_t set, int lane) { return __popcll(set & ((uint64_t(1) << lane) - 1u)); }
constexpr int block_threads(int block) { return block; }
__device__ __forceinline__ void block_sync() { __syncthreads(); }
// one lane's addition to a counter other wavefronts add to as well (an ordinary vector atomic; the plain sum when serial)
__device__ __forceinline__ void wave_atomic_add(int32_t* p, int32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void wave_atomic_or(int32_t* p, int32_t v) { atomicOr(p, v); }
// what one lane stored to global memory before it is what every lane of the wavefront loads after it (the lanes run in
// step; the fence keeps the compiler and the memory pipeline from passing a load ahead of the store)
__device__ __forceinline__ void wave_fence() { __threadfence_block(); }
#endif

// "every lane its share of n items": lanes j, j + 64, ... on the device, all of them in the serial build
#define WAVE_FOR(j, n) for (int j = lane; j < (n); j += WAVE_LANES)

// xor butterflies (32, 16, ... 1): every lane ends with the same bits, and the same bits on every run
MZX_WAVE_FN float wave_max(float v) {
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) v = fmaxf(v, lane_xor(v, o));
  return v;
}
MZX_WAVE_FN float wave_sum(float v) {
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) v = v + lane_xor(v, o);
  return v;
}
MZX_WAVE_FN double wave_sum_f64(double v) {
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) v = v + lane_xor(v, o);
  return v;
}
MZX_WAVE_FN int32_t wave_sum_i32(int32_t v) {
#pragma unroll
  for (int o = WAVE_LANES / 2; o >= 1; o >>= 1) v = v + lane_xor(v, o);
  return v;
}
// inclusive scan over the lanes (lane l ends with v_0 + ... + v_l in a fixed association)
MZX_WAVE_FN double wave_scan_f64(double v, int lane) {
#pragma unroll
  for (int o = 1; o < WAVE_LANES; o <<= 1) {
    const double below = lane_up(v, o);
    if (lane >= o) v = below + v;
  }
  return v;
}

}  // namespace mzx
