// The per-point half of data.radar_map (host statement: data.radar_project), shared by the radar map of a batch
// (csrc/radarmap.hip), the radar map under Mosaic (csrc/mosaic.hip) and the radar readout of the detections
// (csrc/boxradar.hip): all must place a point on the same pixel with the same depth, bit for bit, so the arithmetic is
// written here once.  Float32, one rounding per operation.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

constexpr unsigned long long RM_EMPTY = ~0ULL;    // a key plane's "no candidate"
constexpr int RM_POINT_FLOATS = 7;                // x, y, z, f0, f1, f2, f3

// Point q under the (3, 4) projection P: false when the point is not kept; otherwise (u, v) are its continuous pixel
// coordinates in the original frame and hw its depth, positive and finite.  The radar maps go on from here into a window
// (rm_project); the readout of the detections (csrc/boxradar.hip) compares (u, v) with the boxes as they are
__device__ __forceinline__ bool rm_project_uv(const float* P, const float* q, float min_depth, float& u, float& v, float& hw) {
  const float x = q[0], y = q[1], z = q[2];
  const float hu = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
  const float hv = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
  hw = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
  // a NaN fails every comparison; |h| < Inf rejects the infinities
  if (!(hw >= min_depth) || !(fabsf(hw) < INFINITY) || !(fabsf(hu) < INFINITY) || !(fabsf(hv) < INFINITY)) return false;
  u = hu / hw;
  v = hv / hw;
  return true;
}

// Point q under the (3, 4) projection P of an (ih, iw) frame shown in an nw x nh window (all four positive): false when the
// point is not kept; otherwise (ix, iy) is its window pixel, 0 <= ix < nw, 0 <= iy < nh, and hw its depth, positive and finite
__device__ __forceinline__ bool rm_project(const float* P, const float* q, float min_depth, int ih, int iw, int nw, int nh,
                                           int& ix, int& iy, float& hw) {
  float u, v;
  if (!rm_project_uv(P, q, min_depth, u, v, hw)) return false;
  const float fx = (u * (float)nw) / (float)iw, fy = (v * (float)nh) / (float)ih;
  if (!(fx >= 0.f && fx < (float)nw && fy >= 0.f && fy < (float)nh)) return false;
  ix = (int)floorf(fx);
  iy = (int)floorf(fy);
  return true;
}

// the candidate of point i at depth hw: hw is positive and finite, so its bits order as an unsigned integer
__device__ __forceinline__ unsigned long long rm_key(float hw, int i) {
  return ((unsigned long long)__float_as_uint(hw) << 32) | (unsigned)i;
}
