// What the three frame modes of TrainStep share beyond Pillow's resample arithmetic (resample.h): the plain letterbox
// targets (csrc/traintargets.hip), the single-image augmentation (csrc/augment.hip) and the Mosaic (csrc/mosaic.hip).  Here
// live the colour stage of data.hsv_jitter and the paste epilogue behind it, the row block and one-hot store of the
// segmentation targets, the box rules (the exact coordinate map, the clip and keep test, the compaction of the kept rows),
// the radar pick, and the shape and workspace checks of the augment and Mosaic entry points.  All modes must equal the host
// functions of data.py bit for bit and one another on an identity record, so each rule is written here once.
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

// the end of a vertical-paste thread: pixel r of image b goes through the colour stage when the record asks for it (the
// whole canvas, its padding included, as the reference), then out as canvas bytes and as normalised planes, each when given
__device__ __forceinline__ void paste_store(const ColorLds& c, bool color, unsigned char* v, unsigned char* canvas, float* images,
                                            long b, long HW, long r) {
  const long e = b * HW + r;
  if (color) hsv_jitter_pixel(c, v);
  if (canvas) {
    canvas[e * 3] = v[0];
    canvas[e * 3 + 1] = v[1];
    canvas[e * 3 + 2] = v[2];
  }
  if (images) normalise_store(images, b, HW, r, v);
}

// ---- the segmentation targets: a workgroup's rows and their one-hot store ---------------------------------------------------
constexpr int ST_ROWS = 16;                       // canvas rows of one workgroup
constexpr long ST_LDS_MAX = 64 * 1024;

// dynamic LDS of a seg-targets workgroup: one column and one row index table, and the clamped labels of its rows
__host__ __device__ inline long st_lds_bytes(int H, int W) { return ((long)W + H) * (long)sizeof(int) + (long)ST_ROWS * W; }

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

// the clip to the (W, H) canvas; true: the box keeps more than 1 px on both axes
__device__ __forceinline__ bool box_clip_keep(long long& x1, long long& y1, long long& x2, long long& y2, int W, int H) {
  if (x1 < 0) x1 = 0;
  if (y1 < 0) y1 = 0;
  if (x2 > W) x2 = W;
  if (y2 > H) y2 = H;
  return x2 - x1 > 1 && y2 - y1 > 1;
}

// One chunk of 256 rows, one per thread of the workgroup: the compaction of the kept rows in thread order, by a ballot
// prefix inside a wave and s_wave[4] in LDS across the waves.  base, the rows kept so far, is the same in every thread and
// grows by the chunk's kept rows; returns the row this thread's box goes to, if kept.  The caller stores its row and then
// synchronises, before the next chunk rewrites s_wave
__device__ __forceinline__ int box_compact_slot(bool keep, int& base, int* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int at = base;
  for (int w = 0; w < wave; ++w) at += s_wave[w];
  at += __popcll(mask & ((1ull << lane) - 1ull));
  base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  return at;
}

// data.boxes_xyxy_to_cxcywh for one row: cx, cy, w, h in double, rounded once on the store, and the class
__device__ __forceinline__ void box_store_cxcywh(float* o, long long x1, long long y1, long long x2, long long y2, int c) {
  const double w = (double)(x2 - x1), h = (double)(y2 - y1);
  o[0] = (float)((double)x1 + w / 2);
  o[1] = (float)((double)y1 + h / 2);
  o[2] = (float)w;
  o[3] = (float)h;
  o[4] = (float)c;
}

// the rows behind the count are zero
__device__ __forceinline__ void box_zero_tail(int base, int max_gt, float* out) {
  for (int i = base * 5 + threadIdx.x; i < max_gt * 5; i += 256) out[i] = 0.f;
}

// ---- the radar map -----------------------------------------------------------------------------------------------------------
// window pixel (wx, wy) of an nw x nh window -> its offset in the stored (H, W) map that begins at `first` and is aligned
// with the letterbox window lb_*: the nearest stored pixel under the pixel-centre map, integers only.
// (2 w + 1) lb / (2 n) < lb: inside the letterbox window, which is inside the canvas
__device__ __forceinline__ long radar_pick(long first, int wx, int wy, int nw, int nh, int lb_nw, int lb_nh, int lb_dx, int lb_dy,
                                           int W) {
  const int sy = lb_dy + (int)(((2LL * wy + 1) * lb_nh) / (2LL * nh));
  const int sx = lb_dx + (int)(((2LL * wx + 1) * lb_nw) / (2LL * nw));
  return first + (long)sy * W + sx;
}

// ---- the entry points' checks ------------------------------------------------------------------------------------------------
// B output images on an H x W canvas from (ihm, iwm) slots: what every augment and Mosaic entry point asks of them
inline bool fm_shape_ok(int B, int ihm, int iwm, int H, int W) {
  return B > 0 && B < 65536 && ihm > 0 && iwm > 0 && H > 0 && W > 0 && H < (1 << 24) && W < (1 << 24);
}

// The frames workspace: `sets` table sets of lb_ragged_slot_ints each, then as many (ihm, W, 3) horizontal results, both
// aligned.  fm_workspace_bytes is what a caller must bring; fm_split_workspace hands out the two parts, or sets the error
inline long fm_tables_bytes(long sets, int H, int W, int cap) { return lb_align(sets * lb_ragged_slot_ints(H, W, cap) * (long)sizeof(int)); }
inline long fm_workspace_bytes(long sets, int ihm, int H, int W, int cap) {
  return fm_tables_bytes(sets, H, W, cap) + lb_align(sets * ihm * W * 3);
}
inline bool fm_split_workspace(const char* who, void* workspace, long bytes, long sets, int ihm, int H, int W, int cap, int*& tables,
                               unsigned char*& mid) {
  const long need = fm_workspace_bytes(sets, ihm, H, W, cap);
  if (!workspace || bytes < need) {
    vr_set_error("%s: workspace %ld < %ld bytes", who, workspace ? bytes : 0L, need);
    return false;
  }
  tables = static_cast<int*>(workspace);
  mid = static_cast<unsigned char*>(workspace) + fm_tables_bytes(sets, H, W, cap);
  return true;
}
