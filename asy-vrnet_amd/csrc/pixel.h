// Per-pixel rules that more than one frame op applies, each written once: Pillow's blend of one byte (render.hip's
// mix_type 0, heatmap.hip's overlay) and the OpenCV INTER_LINEAR tap of one axis (segpost.hip's class map, heatmap.hip's
// mask).  Both state their arithmetic operation by operation, so contraction is off inside each body, whatever the
// including file sets: an FMA rounds once and gives other bytes / can move floor() across an integer.
#pragma once
#include "common.h"

// ImagingBlend (Blend.c) on one byte
__device__ __forceinline__ unsigned int blend_byte(unsigned int a, unsigned int b, float alpha) {
#pragma clang fp contract(off)
  const float d = (float)((int)b - (int)a);
  const float t = alpha * d;
  const float v = (float)a + t;
  return (unsigned int)(int)v & 255u;
}

// OpenCV resize INTER_LINEAR source coordinate along one axis: f = (d + 0.5) * scale - 0.5, s = floor(f), f -= s, clamped
// to the first / last source pixel with weight 0 on the second tap.
__device__ __forceinline__ void linear_tap(int d, float scale, int src, int& s0, int& s1, float& f) {
#pragma clang fp contract(off)
  f = ((float)d + 0.5f) * scale - 0.5f;
  const float fl = floorf(f);
  int s = (int)fl;
  f = f - fl;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  s0 = s;
  s1 = s + 1 < src ? s + 1 : s;
}
