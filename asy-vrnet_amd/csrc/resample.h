// Pillow's 8-bit resample arithmetic (Resample.c) and the stores behind it, shared by the letterbox (csrc/letterbox.hip), the
// training augmentation (csrc/augment.hip) and the Mosaic (csrc/mosaic.hip): all must produce Pillow's bytes, so all use
// these functions and nothing of their own.  Every double / float operation rounds once (contract off), as the C code Pillow compiles to does.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

constexpr int LB_PRECISION_BITS = 32 - 8 - 2;      // Resample.c PRECISION_BITS

// Resample.c bicubic_filter, a = -0.5
__device__ __forceinline__ double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for output index xx of an axis resized in -> out, stored as entry
// `at` of a table whose taps are `stride` entries apart: bounds[2 at], bounds[2 at + 1] = (xmin, n), taps k[t * stride + at]
__device__ inline void bicubic_taps_at(int xx, int in, int out, int cap, int* bounds, int* k, int at, int stride) {
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  int n = xmax - xmin;
  // keeps the stores inside the table.  Never taken from vrnet_letterbox_u8, whose cap is this axis's own ksize >= n; the
  // ragged callers' cap is the pipeline's max_taps, which a wrong table can exceed: the taps are then truncated and the
  // tables kernel reports FLAG_GEOMETRY
  if (n > cap) n = cap;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < n; ++x) {
    double w = bicubic((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[(long)x * stride + at] = w < 0 ? (int)(-0.5 + w * (1 << LB_PRECISION_BITS)) : (int)(0.5 + w * (1 << LB_PRECISION_BITS));
  }
  bounds[2 * at] = xmin;
  bounds[2 * at + 1] = n;
}

// the table of a whole axis: entry xx of out
__device__ inline void bicubic_taps(int xx, int in, int out, int cap, int* bounds, int* k) {
  bicubic_taps_at(xx, in, out, cap, bounds, k, xx, out);
}

__device__ __forceinline__ unsigned char clip8(int acc) {
  acc >>= LB_PRECISION_BITS;
  return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

// ImagingResampleHorizontal_8bpc / Vertical_8bpc for the three channels of one output pixel: tap t reads src[t * step + c]
// with weight k[t * kstride]; v receives the rounded, clipped bytes.  step is 3 along a row, -3 along a mirrored row, a
// row's bytes down a column; Step is the caller's own index type (int or long), so its address arithmetic stays as it was
template <typename Step>
__device__ __forceinline__ void resample_taps3(const unsigned char* src, Step step, const int* k, int kstride, int n,
                                               unsigned char* v) {
  int a0 = 1 << (LB_PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int w = k[(long)t * kstride];
    a0 += w * src[t * step];
    a1 += w * src[t * step + 1];
    a2 += w * src[t * step + 2];
  }
  v[0] = clip8(a0);
  v[1] = clip8(a1);
  v[2] = clip8(a2);
}

// batch_formats_kernel's arithmetic: ((v / 255) - mean) / std in double, rounded once; pixel r of image b's CHW planes
__device__ __forceinline__ void normalise_store(float* images, long b, long HW, long r, const unsigned char* v) {
  const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double d = (double)v[c];
    d /= 255.0;
    d -= mean[c];
    d /= sd[c];
    images[(b * 3 + c) * HW + r] = (float)d;
  }
}

// vr_nearest_indices for the entries [first, first + count) of the axis only: the recurrence is a running sum from index
// 0, so it runs from there and keeps what the caller can see (idx[x - first])
__device__ inline void vr_nearest_indices_from(int in, int out, int first, int count, int* idx) {
  const double a0 = (double)in / out;
  double xo = a0 * 0.5;
  for (int x = 0; x < first + count; ++x) {
    if (x >= first) idx[x - first] = (int)xo;
    xo += a0;
  }
}

// Resample.c precompute_coeffs: ksize, the tap capacity of one output index
__host__ __device__ inline int lb_ksize(int in, int out) {
  double fs = (double)in / out;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(2.0 * fs) * 2 + 1;
}

inline long lb_align(long n) { return (n + 255) / 256 * 256; }

// ints of one image's tables in the ragged workspace: bounds and taps of W columns and H rows, and their nearest indices
__host__ __device__ inline long lb_ragged_slot_ints(int H, int W, int cap) { return ((long)W + H) * (3 + cap); }
