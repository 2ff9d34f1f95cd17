// Integer sums and scans over a wave and over a workgroup, each written once for the frame-stage kernels (crops, regions,
// dehaze, box radar, tracking, JPEG).  ONE ASSUMPTION, stated here for all of them: the workgroup is one-dimensional with
// VR_WG_THREADS = 256 threads, four waves of 64, and every thread of it makes the call.  Integral types only: a sum of
// integers does not depend on its order, one of floats does (the float reductions of the other files stay where they are).
//
// The workgroup forms pass the wave results through four LDS slots of the caller and hold ONE barrier, between the write
// of the slots and their read; they have NO leading barrier.  A caller that uses the same slots twice puts its own
// __syncthreads() between the calls, so that no wave rewrites a slot another one still reads.
#pragma once
#include "common.h"

#include <type_traits>

constexpr int VR_WG_THREADS = 256, VR_WG_WAVES = VR_WG_THREADS / 64;

struct vr_op_sum {
  template <typename T>
  __device__ __forceinline__ static T apply(T a, T b) { return a + b; }
};
struct vr_op_max {
  template <typename T>
  __device__ __forceinline__ static T apply(T a, T b) { return a > b ? a : b; }
};

// __shfl_xor of a 64-bit key as two 32-bit halves
__device__ __forceinline__ unsigned long long vr_shfl_xor64(unsigned long long k, int o) {
  const unsigned lo = __shfl_xor((unsigned)k, o, 64), hi = __shfl_xor((unsigned)(k >> 32), o, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// the sum over the wave, in every lane
template <typename T>
__device__ __forceinline__ T vr_wave_sum(T v) {
  static_assert(std::is_integral<T>::value, "integral types only");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the inclusive scan over the lanes of a wave: lane l gets Op (the sum unless named) over the lanes 0..l
template <typename Op = vr_op_sum, typename T>
__device__ __forceinline__ T vr_wave_scan_incl(T v) {
  static_assert(std::is_integral<T>::value, "integral types only");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v = Op::apply(v, u);
  }
  return v;
}

// the inclusive scan over the workgroup in thread order, and Op over all of it in `total`
template <typename Op, typename T>
__device__ __forceinline__ T vr_block_scan_incl(T v, T* s_wave, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = vr_wave_scan_incl<Op>(v);
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < VR_WG_WAVES - 1; ++w)
    if (w < wave) v = Op::apply(v, s_wave[w]);
  total = Op::apply(Op::apply(s_wave[0], s_wave[1]), Op::apply(s_wave[2], s_wave[3]));
  return v;
}

// the sum over the workgroup, in every thread
template <typename T>
__device__ __forceinline__ T vr_block_sum(T v, T* s_wave) {
  v = vr_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
}
