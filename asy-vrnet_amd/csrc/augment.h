// What the single-image augmentation (csrc/augment.hip) and the Mosaic (csrc/mosaic.hip) share beyond Pillow's resample
// arithmetic (resample.h): the colour stage of data.hsv_jitter, the exact box-coordinate map, and the row block and one-hot
// store of the segmentation targets.  Both must equal the host functions of data.py bit for bit, so both use these
// functions and nothing of their own.
#pragma once
#include "resample.h"

#pragma clang fp contract(off)

// ---- the colour stage: data.hsv_jitter for one pixel ---------------------------------------------------------------------
constexpr int HSV_SHIFT = 12;

struct ColorLds {
  int sdiv[256], hdiv[256];          // rint((255 << 12) / i), rint((180 << 12) / (6 i)); 0 at i = 0
  unsigned char lut[3][256];
};

// Fills c in a workgroup of 256 threads from the 768 table bytes of a record (4-byte aligned words), and synchronises
__device__ __forceinline__ void color_lds_fill(ColorLds& c, const unsigned* lut) {
  const int i = threadIdx.x;
  c.sdiv[i] = i ? (int)rint((double)(255 << HSV_SHIFT) / (double)i) : 0;
  c.hdiv[i] = i ? (int)rint((double)(180 << HSV_SHIFT) / (6.0 * (double)i)) : 0;
  if (i < 192) reinterpret_cast<unsigned*>(&c.lut[0][0])[i] = lut[i];
  __syncthreads();
}

__device__ __forceinline__ void hsv_jitter_pixel(const ColorLds& c, unsigned char* px) {
  const int r = px[0], g = px[1], b = px[2];
  const int v = max(r, max(g, b)), vmin = min(r, min(g, b)), d = v - vmin;
  const int s = (d * c.sdiv[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT;
  const int h0 = v == r ? g - b : (v == g ? b - r + 2 * d : r - g + 4 * d);
  int h = (h0 * c.hdiv[d] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT;          // arithmetic shift
  if (h < 0) h += 180;
  const int h8 = c.lut[0][h & 255], s8 = c.lut[1][s > 255 ? 255 : s], v8 = c.lut[2][v];
  const float fv = (float)v8 * (1.f / 255.f);
  float fb = fv, fg = fv, fr = fv;
  if (s8 != 0) {
    const float fs = (float)s8 * (1.f / 255.f);
    float fh = (float)h8 * (6.f / 180.f);
    if (fh >= 6.f) fh -= 6.f;                      // a table value >= 180: the hue wraps (exact: 6 <= fh < 12)
    const float fl = floorf(fh);
    const int sector = (int)fl;                    // 0 .. 5
    const float f = fh - fl;
    // sector -> the tab entries of (b, g, r): {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}, two bits per sector; picked by
    // selects, so tab stays in registers
    const unsigned ib = 0x835u >> (2 * sector) & 3u;            // 1,1,3,0,0,2
    const unsigned ig = 0x583u >> (2 * sector) & 3u;            // 3,0,0,2,1,1
    const unsigned ir = 0x358u >> (2 * sector) & 3u;            // 0,2,1,1,3,0
    const float t0 = fv, t1 = fv * (1.f - fs), t2 = fv * (1.f - fs * f), t3 = fv * (1.f - fs * (1.f - f));
    fb = ib == 0 ? t0 : (ib == 1 ? t1 : (ib == 2 ? t2 : t3));
    fg = ig == 0 ? t0 : (ig == 1 ? t1 : (ig == 2 ? t2 : t3));
    fr = ir == 0 ? t0 : (ir == 1 ? t1 : (ir == 2 ? t2 : t3));
  }
  const float o[3] = {fr, fg, fb};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int q = (int)__builtin_rintf(o[k] * 255.f);
    px[k] = (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
  }
}

// ---- the segmentation targets: a workgroup's rows and their one-hot store ---------------------------------------------------
constexpr int ST_ROWS = 16;                       // canvas rows of one workgroup
constexpr long ST_LDS_MAX = 64 * 1024;

// cls (npix clamped labels in LDS, complete) -> oh (npix, n1) one-hot floats, by a workgroup of 256 threads; vec4: npix * n1
// is a multiple of 4 and oh is 16-byte aligned, so every chunk is a whole float4
__device__ __forceinline__ void st_store_onehot(const unsigned char* cls, float* oh, int npix, int n1, int vec4) {
  const int total = npix * n1;
  if (vec4) {
    for (int q = threadIdx.x; q < total / 4; q += 256) {
      int px = (q * 4) / n1, c = q * 4 - px * n1, lab = cls[px];
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = c == lab ? 1.f : 0.f;
        if (++c == n1 && j < 3) {
          c = 0;
          lab = cls[++px];
        }
      }
      *reinterpret_cast<f32x4*>(oh + q * 4) = v;
    }
  } else {
    for (int f = threadIdx.x; f < total; f += 256) {
      const int px = f / n1;
      oh[f] = f - px * n1 == cls[px] ? 1.f : 0.f;
    }
  }
}

// ---- the box targets ---------------------------------------------------------------------------------------------------------
// out[:, k] * n / i + d assigned back into the integer array (dataloader.py:239-240): numpy multiplies in int64, divides
// in double (true_divide), adds the offset in double and truncates toward zero on the store
__device__ __forceinline__ long long map_coord(long long v, int n, int i, int d) {
  double t = (double)(v * (long long)n);
  t /= (double)i;
  t += (double)d;
  return (long long)t;
}
