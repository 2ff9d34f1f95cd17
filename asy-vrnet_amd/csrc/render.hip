// Result rendering on the device, from the bytes that are already there: the picture deeplab.py:169-222 `detect_image` makes
// of the class map (three mix_types and the per-class pixel counts of :172-185) and the box outlines of yolo.py:221-222, in
// ONE launch over the original frames.
//   mix_type 1  out = palette[class]                                                    (deeplab.py:209)
//   mix_type 2  out = frame where class != 0, else 0                                    (deeplab.py:216: a bool times float32)
//   mix_type 0  Image.blend(frame, palette[class], alpha): Pillow's ImagingBlend per byte,
//               out = (uint8)((float)a + alpha * (float)((int)b - (int)a)), a = frame byte, b = palette byte, alpha a C float,
//               every operation rounded to fp32 (contract off: an FMA rounds once and gives other bytes), truncated
//   no class map  out = frame
//   boxes       painted after the mix, as the reference draws them after the network ran: for row r of image b and
//               i = 0 .. thickness-1 the ring [left+i, top+i, right-i, bottom-i] paints the perimeter of that inclusive
//               rectangle, clipped to the image, while left+i <= right-i and top+i <= bottom-i.  Pixel (x, y) lies on ring
//               d = min(x-left, right-x, y-top, bottom-y) if d >= 0 and on no other, so it is painted iff 0 <= d < thickness.
//               Where several rows of an image paint a pixel the LAST row wins (sequential drawing): every pixel scans
//               its image's rows, kept in LDS, from the last to the first and stops at the first hit -- no racing stores,
//               the result does not depend on scheduling.
//               Two differences from ImageDraw.rectangle(outline=) of Pillow 12.2: Pillow paints a one-row ring (y0 == y1)
//               two rows high ([5,5,5,5] paints (5,5) and (5,6)) and raises ValueError for x1 < x0; here a ring is its
//               geometric perimeter and an empty ring paints nothing.
// A flat grid-stride loop over the B*ih*iw pixels of the contiguous tensors, four pixels per thread: one dword of class ids
// and three dwords of frame bytes in, three dwords out.  The leading pixels up to dword alignment and the total % 4 tail go
// bytewise; tensors whose addresses do not share one alignment go bytewise as a whole.  Palettes and the image's box rows
// sit in LDS.  The counts use a per-workgroup LDS histogram of the image the workgroup is in, flushed with one 64-bit
// integer atomic per non-empty bin when the workgroup moves to the next image (segpost.hip's hist scheme); the pixels of
// an iteration that straddles into the next image add to global memory directly.  Integer atomics only: the same counts
// on every run.
// Data errors do not stop the launch: a class id >= n_colors takes the last colour and is not counted, a colour index
// outside [0, n_box_colors) is clamped, rows past RN_MAXBOX of one image are ignored, and each sets its bit in *flag.
#include "common.h"
#include "pixel.h"                   // blend_byte: ImagingBlend on one byte, shared with heatmap.hip

#pragma clang fp contract(off)

namespace {

constexpr int RN_MAXCOL = 256;
constexpr int RN_MAXBOX = 1024;      // box rows of ONE image
constexpr int RN_COORD = 1 << 29;    // coordinates are clamped to +-2^29: with ih, iw, thickness <= 2^24 no difference overflows
                                     // and a clamped edge stays further than `thickness` from every pixel
constexpr int RN_FLAG_CLASS = 1, RN_FLAG_BOX_COLOUR = 2, RN_FLAG_BOX_ROWS = 4;

struct RenderArgs {
  const unsigned char* frames;       // (B, ih, iw, 3)
  const unsigned char* cmap;         // (B, ih, iw) or null
  const unsigned char* palette;      // (n_colors, 3) or null
  const int* boxes;                  // (n_rows, 5) or null
  const int* offsets;                // (B + 1)
  const unsigned char* box_palette;  // (n_box_colors, 3)
  unsigned char* out;                // (B, ih, iw, 3)
  unsigned long long* counts;        // (B, n_colors) or null
  int* flag;                         // or null
  int B, ih, iw, n_colors, n_box_colors, n_rows, thickness, mix;
  int vec;                           // the groups use dword accesses
  int inplace;                       // out == frames and no class map: only painted pixels are written
  int head, ngroups, total;          // pixels [0, head) and [head + 4 ngroups, total) go one by one
  float alpha;
};

__device__ __forceinline__ int4 load_row(const int* row, int& colour) {
  colour = row[4];
  return make_int4(vr_clampi(row[0], -RN_COORD, RN_COORD), vr_clampi(row[1], -RN_COORD, RN_COORD),
                   vr_clampi(row[2], -RN_COORD, RN_COORD), vr_clampi(row[3], -RN_COORD, RN_COORD));
}

// first and one-past-last row of image b, kept inside the rows array whatever the offsets hold
__device__ __forceinline__ void row_range(const RenderArgs& p, int b, int& start, int& n) {
  start = 0;
  n = 0;
  if (!p.boxes) return;
  vr_row_range(p.offsets, b, p.n_rows, start, n);
}

__device__ __forceinline__ void raise_flag(const RenderArgs& p, int bit) {
  if (p.flag) atomicOr(p.flag, bit);
}

__device__ __forceinline__ unsigned int pack_rgb(const unsigned char* c) {
  return (unsigned int)c[0] | ((unsigned int)c[1] << 8) | ((unsigned int)c[2] << 16);
}

// the pixel before the boxes: frame and colour as packed r | g << 8 | b << 16
__device__ __forceinline__ unsigned int shade(const RenderArgs& p, bool has_map, int cls, unsigned int frame, unsigned int colour) {
  if (!has_map) return frame;
  if (p.mix == 1) return colour;
  if (p.mix == 2) return cls != 0 ? frame : 0u;
  return blend_byte(frame & 255u, colour & 255u, p.alpha) | (blend_byte((frame >> 8) & 255u, (colour >> 8) & 255u, p.alpha) << 8) |
         (blend_byte((frame >> 16) & 255u, (colour >> 16) & 255u, p.alpha) << 16);
}

__device__ __forceinline__ bool on_rings(int x, int y, const int4 q, int thickness) {
  const int dx = min(x - q.x, q.z - x), dy = min(y - q.y, q.w - y);
  return (unsigned int)min(dx, dy) < (unsigned int)thickness;
}

// One pixel on its own (head, tail, a group that wraps a row, a pixel of another image than the workgroup's): box rows from
// global memory, counts straight to global memory.
__device__ void render_pixel(const RenderArgs& p, const unsigned int* s_pal, const unsigned int* s_bpal, int pix) {
  const int HW = p.ih * p.iw;
  const int b = pix / HW, r = pix - b * HW, y = r / p.iw, x = r - y * p.iw;
  const bool has_map = p.cmap != nullptr;
  int cls = 0;
  unsigned int colour = 0;
  if (has_map) {
    cls = p.cmap[pix];
    int c = cls;
    if (p.n_colors > 0 && c >= p.n_colors) {
      raise_flag(p, RN_FLAG_CLASS);
      c = p.n_colors - 1;
    } else if (p.counts) {
      atomicAdd(&p.counts[(long)b * p.n_colors + c], 1ull);
    }
    colour = s_pal[c & 255];
  }
  const unsigned char* f = p.frames + 3L * pix;
  const bool need_frame = has_map ? p.mix != 1 : !p.inplace;
  unsigned int v = shade(p, has_map, cls, need_frame ? pack_rgb(f) : 0u, colour);
  int start, n;
  row_range(p, b, start, n);
  if (n > RN_MAXBOX) n = RN_MAXBOX;
  bool painted = false;
  for (int k = n - 1; k >= 0; --k) {
    int ci;
    const int4 q = load_row(p.boxes + 5L * (start + k), ci);
    if (on_rings(x, y, q, p.thickness)) {
      v = s_bpal[vr_clampi(ci, 0, p.n_box_colors - 1)];
      painted = true;
      break;
    }
  }
  if (p.inplace && !painted) return;
  unsigned char* o = p.out + 3L * pix;
  o[0] = (unsigned char)v;
  o[1] = (unsigned char)(v >> 8);
  o[2] = (unsigned char)(v >> 16);
}

__global__ __launch_bounds__(256) void render_kernel(const RenderArgs p) {
  __shared__ int4 s_rows[RN_MAXBOX];
  __shared__ unsigned char s_rcol[RN_MAXBOX];
  __shared__ unsigned int s_pal[RN_MAXCOL], s_bpal[RN_MAXCOL], s_bins[RN_MAXCOL];
  const int tid = threadIdx.x;
  const int HW = p.ih * p.iw;
  const bool has_map = p.cmap != nullptr;
  for (int i = tid; i < RN_MAXCOL; i += 256) {
    s_pal[i] = (p.palette && i < p.n_colors) ? pack_rgb(p.palette + 3 * i) : 0u;
    s_bpal[i] = (p.box_palette && i < p.n_box_colors) ? pack_rgb(p.box_palette + 3 * i) : 0u;
    s_bins[i] = 0u;
  }
  int cur_b = -1, nrows = 0;
  for (int g0 = blockIdx.x * 256; g0 < p.ngroups; g0 += gridDim.x * 256) {
    const int pb = (p.head + 4 * g0) / HW;          // the image of this iteration's first pixel: the same for every thread
    if (pb != cur_b) {
      __syncthreads();
      if (p.counts && cur_b >= 0)
        for (int i = tid; i < p.n_colors; i += 256) {
          const unsigned int v = s_bins[i];
          if (v) atomicAdd(&p.counts[(long)cur_b * p.n_colors + i], (unsigned long long)v);
          s_bins[i] = 0u;
        }
      int start;
      row_range(p, pb, start, nrows);
      if (nrows > RN_MAXBOX) {
        if (tid == 0) raise_flag(p, RN_FLAG_BOX_ROWS);
        nrows = RN_MAXBOX;
      }
      for (int k = tid; k < nrows; k += 256) {
        int ci;
        s_rows[k] = load_row(p.boxes + 5L * (start + k), ci);
        if (ci < 0 || ci >= p.n_box_colors) raise_flag(p, RN_FLAG_BOX_COLOUR);
        s_rcol[k] = (unsigned char)vr_clampi(ci, 0, p.n_box_colors - 1);
      }
      cur_b = pb;
      __syncthreads();
    }
    const int g = g0 + tid;
    if (g >= p.ngroups) continue;
    const int p0 = p.head + 4 * g;
    const int b = p0 / HW, r = p0 - b * HW, y = r / p.iw, x = r - y * p.iw;
    if (b != cur_b || x + 3 >= p.iw) {              // wraps a row or lies in the next image: pixel by pixel
      for (int j = 0; j < 4; ++j) render_pixel(p, s_pal, s_bpal, p0 + j);
      continue;
    }
    // ---- four pixels of one row of image cur_b
    unsigned int cls4 = 0;
    if (has_map) {
      const unsigned char* c = p.cmap + p0;
      cls4 = p.vec ? *reinterpret_cast<const unsigned int*>(c)
                   : ((unsigned int)c[0] | ((unsigned int)c[1] << 8) | ((unsigned int)c[2] << 16) | ((unsigned int)c[3] << 24));
    }
    unsigned int f[3] = {0u, 0u, 0u};
    if (has_map ? p.mix != 1 : !p.inplace) {
      const unsigned char* s = p.frames + 3L * p0;
      if (p.vec) {
        const unsigned int* s4 = reinterpret_cast<const unsigned int*>(s);
        f[0] = s4[0];
        f[1] = s4[1];
        f[2] = s4[2];
      } else {
#pragma unroll
        for (int j = 0; j < 12; ++j) f[j >> 2] |= (unsigned int)s[j] << (8 * (j & 3));
      }
    }
    // the 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 as four packed pixels
    unsigned int px[4] = {f[0] & 0xFFFFFFu, (f[0] >> 24) | ((f[1] & 0xFFFFu) << 8), (f[1] >> 16) | ((f[2] & 0xFFu) << 16), f[2] >> 8};
    if (has_map) {
      int cls[4];
      bool bad = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cls[j] = (cls4 >> (8 * j)) & 255;
        int c = cls[j];
        if (p.n_colors > 0 && c >= p.n_colors) {
          bad = true;
          c = p.n_colors - 1;
        }
        px[j] = shade(p, true, cls[j], px[j], s_pal[c]);
      }
      if (bad) raise_flag(p, RN_FLAG_CLASS);
      if (p.counts) {
        // a wave inside one region of the map adds once; otherwise a thread whose four pixels agree adds once
        const bool same4 = cls[0] == cls[1] && cls[0] == cls[2] && cls[0] == cls[3] && !bad;
        const int first = __builtin_amdgcn_readfirstlane(cls[0]);
        if (__all(same4 && cls[0] == first)) {
          const unsigned long long active = __ballot(1);
          if (__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&s_bins[first], 4u * (unsigned int)__popcll(active));
        } else if (same4) {
          atomicAdd(&s_bins[cls[0]], 4u);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (cls[j] < p.n_colors) atomicAdd(&s_bins[cls[j]], 1u);
        }
      }
    }
    unsigned int hit = 0;                            // bit j: pixel j is painted
    for (int k = nrows - 1; k >= 0 && hit != 15u; --k) {
      const int4 q = s_rows[k];
      const int dy = min(y - q.y, q.w - y);
      if (dy < 0) continue;                          // the row misses the box
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int dx = min(x + j - q.x, q.z - (x + j));
        if (!(hit & (1u << j)) && (unsigned int)min(dx, dy) < (unsigned int)p.thickness) {
          px[j] = s_bpal[s_rcol[k]];
          hit |= 1u << j;
        }
      }
    }
    unsigned char* o = p.out + 3L * p0;
    if (p.inplace) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (hit & (1u << j)) {
          o[3 * j] = (unsigned char)px[j];
          o[3 * j + 1] = (unsigned char)(px[j] >> 8);
          o[3 * j + 2] = (unsigned char)(px[j] >> 16);
        }
      continue;
    }
    const unsigned int o0 = px[0] | (px[1] << 24), o1 = (px[1] >> 8) | (px[2] << 16), o2 = (px[2] >> 16) | (px[3] << 8);
    if (p.vec) {
      unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
      o4[0] = o0;
      o4[1] = o1;
      o4[2] = o2;
    } else {
      const unsigned int w[3] = {o0, o1, o2};
#pragma unroll
      for (int j = 0; j < 12; ++j) o[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
  __syncthreads();
  if (p.counts && cur_b >= 0)
    for (int i = tid; i < p.n_colors; i += 256) {
      const unsigned int v = s_bins[i];
      if (v) atomicAdd(&p.counts[(long)cur_b * p.n_colors + i], (unsigned long long)v);
    }
  // the pixels outside the groups: at most 3 in front and 3 behind
  if (blockIdx.x == 0) {
    const int nedge = p.total - 4 * p.ngroups;
    if (tid < nedge) render_pixel(p, s_pal, s_bpal, tid < p.head ? tid : 4 * p.ngroups + tid);
  }
}

// ---- the ragged form: frames, class map and out are (B, ihm, iwm[, 3]) slots with image b in the top-left ih_b x iw_b
// corner; ih_b, iw_b and the outline thickness come from tab[b].  blockIdx.y is the image, so a workgroup keeps one
// image's box rows and one histogram in LDS for its whole life.  Four consecutive pixels of the slot per thread (dword
// accesses when the slots allow it), each with its own (x, y): a group may wrap a row.  Every pixel of the slot outside
// the image is written 0 and counts nowhere.
// A kernel of its own, unlike the letterbox and seg_predict: render_kernel draws in place, keeps dword accesses for any
// base alignment through a head of 0-3 pixels and has a one-row shortcut in the ring scan; this one falls back to byte
// accesses when ihm * iwm % 4 != 0 and B > 1.  Each is better on some input.
struct RaggedRenderArgs {
  RenderArgs r;                      // ih, iw = the slot ihm, iwm; thickness, head, ngroups, total, inplace unused
  const vrnet_frame_geom* tab;       // (B)
};

__global__ __launch_bounds__(256) void render_ragged_kernel(const RaggedRenderArgs a) {
  __shared__ int4 s_rows[RN_MAXBOX];
  __shared__ unsigned char s_rcol[RN_MAXBOX];
  __shared__ unsigned int s_pal[RN_MAXCOL], s_bpal[RN_MAXCOL], s_bins[RN_MAXCOL];
  const RenderArgs& p = a.r;
  const int tid = threadIdx.x, b = blockIdx.y;
  const bool has_map = p.cmap != nullptr, first = blockIdx.x == 0 && tid == 0;
  bool bad;
  const vrnet_frame_geom g = vr_geom_load(a.tab, b, p.ih, p.iw, 0, 0, bad);
  if (bad && first) raise_flag(p, VR_FLAG_GEOMETRY);
  for (int i = tid; i < RN_MAXCOL; i += 256) {
    s_pal[i] = (p.palette && i < p.n_colors) ? pack_rgb(p.palette + 3 * i) : 0u;
    s_bpal[i] = (p.box_palette && i < p.n_box_colors) ? pack_rgb(p.box_palette + 3 * i) : 0u;
    s_bins[i] = 0u;
  }
  int start, nrows;
  row_range(p, b, start, nrows);
  if (nrows > RN_MAXBOX) {
    if (first) raise_flag(p, RN_FLAG_BOX_ROWS);
    nrows = RN_MAXBOX;
  }
  for (int k = tid; k < nrows; k += 256) {
    int ci;
    s_rows[k] = load_row(p.boxes + 5L * (start + k), ci);
    if (ci < 0 || ci >= p.n_box_colors) raise_flag(p, RN_FLAG_BOX_COLOUR);
    s_rcol[k] = (unsigned char)vr_clampi(ci, 0, p.n_box_colors - 1);
  }
  __syncthreads();
  const int slot = p.ih * p.iw, ngroups = (slot + 3) / 4;
  const long base = (long)b * slot;
  const bool need_frame = has_map ? p.mix != 1 : true;
  for (int grp = blockIdx.x * 256 + tid; grp < ngroups; grp += gridDim.x * 256) {
    const int p0 = 4 * grp, npx = min(4, slot - p0);
    const bool dwords = p.vec && npx == 4;
    unsigned int cls4 = 0;
    if (has_map) {
      const unsigned char* c = p.cmap + base + p0;
      if (dwords) cls4 = *reinterpret_cast<const unsigned int*>(c);
      else
        for (int j = 0; j < npx; ++j) cls4 |= (unsigned int)c[j] << (8 * j);
    }
    unsigned int f[3] = {0u, 0u, 0u};
    if (need_frame) {
      const unsigned char* s = p.frames + 3L * (base + p0);
      if (dwords) {
        const unsigned int* s4 = reinterpret_cast<const unsigned int*>(s);
        f[0] = s4[0];
        f[1] = s4[1];
        f[2] = s4[2];
      } else {
        for (int j = 0; j < 3 * npx; ++j) f[j >> 2] |= (unsigned int)s[j] << (8 * (j & 3));
      }
    }
    unsigned int px[4] = {f[0] & 0xFFFFFFu, (f[0] >> 24) | ((f[1] & 0xFFFFu) << 8), (f[1] >> 16) | ((f[2] & 0xFFu) << 16), f[2] >> 8};
    int xs[4], ys[4];
    unsigned int in = 0;                               // bit j: pixel j lies inside the image
    {
      int y = p0 / p.iw, x = p0 - y * p.iw;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xs[j] = x;
        ys[j] = y;
        if (j < npx && y < g.ih && x < g.iw) in |= 1u << j;
        if (++x == p.iw) { x = 0; ++y; }
      }
    }
    if (has_map) {
      int cls[4];
      bool badcls = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        cls[j] = (cls4 >> (8 * j)) & 255;
        int c = cls[j];
        if (p.n_colors > 0 && c >= p.n_colors) {
          if (in & (1u << j)) badcls = true;
          c = p.n_colors - 1;
        }
        px[j] = shade(p, true, cls[j], px[j], s_pal[c]);
      }
      if (badcls) raise_flag(p, RN_FLAG_CLASS);
      if (p.counts) {
        // a wave inside one region of the map adds once; otherwise a thread whose four pixels agree adds once
        const bool same4 = in == 15u && cls[0] == cls[1] && cls[0] == cls[2] && cls[0] == cls[3] && !badcls;
        const int lead = __builtin_amdgcn_readfirstlane(cls[0]);
        if (__all(same4 && cls[0] == lead)) {
          const unsigned long long active = __ballot(1);
          if (__lane_id() == __ffsll((long long)active) - 1) atomicAdd(&s_bins[lead], 4u * (unsigned int)__popcll(active));
        } else if (same4) {
          atomicAdd(&s_bins[cls[0]], 4u);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if ((in & (1u << j)) && cls[j] < p.n_colors) atomicAdd(&s_bins[cls[j]], 1u);
        }
      }
    }
    unsigned int hit = ~in & 15u;                      // bit j: pixel j is settled (painted, or padding)
    for (int k = nrows - 1; k >= 0 && hit != 15u; --k) {
      const int4 q = s_rows[k];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!(hit & (1u << j)) && on_rings(xs[j], ys[j], q, g.thickness)) {
          px[j] = s_bpal[s_rcol[k]];
          hit |= 1u << j;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (!(in & (1u << j))) px[j] = 0u;
    unsigned char* o = p.out + 3L * (base + p0);
    const unsigned int o0 = px[0] | (px[1] << 24), o1 = (px[1] >> 8) | (px[2] << 16), o2 = (px[2] >> 16) | (px[3] << 8);
    if (dwords) {
      unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
      o4[0] = o0;
      o4[1] = o1;
      o4[2] = o2;
    } else {
      const unsigned int w[3] = {o0, o1, o2};
      for (int j = 0; j < 3 * npx; ++j) o[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
  __syncthreads();
  if (p.counts)
    for (int i = tid; i < p.n_colors; i += 256) {
      const unsigned int v = s_bins[i];
      if (v) atomicAdd(&p.counts[(long)b * p.n_colors + i], (unsigned long long)v);
    }
}

bool overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

// the argument checks that both entry points share; `ok`: the entry point's own pointer and batch conditions, `what`
// names the size h x w in the message
int render_check(const char* fn, bool ok, const char* what, int B, int h, int w, const unsigned char* class_map,
                 const unsigned char* palette, int n_colors, int mix_type, float alpha, const long long* counts) {
  VR_CHECK_ARG(ok && B > 0 && h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24) && (long)B * h * w < (1L << 31),
               "%s: bad shape (B %d, %s %d x %d; at most 2^31 - 1 pixels in all)", fn, B, what, h, w);
  VR_CHECK_ARG(mix_type >= 0 && mix_type <= 2, "%s: mix_type %d is not 0, 1 or 2", fn, mix_type);
  VR_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha %g outside [0, 1]", fn, (double)alpha);
  VR_CHECK_ARG(n_colors >= 0 && n_colors <= RN_MAXCOL && (n_colors > 0) == (palette != nullptr || counts != nullptr) &&
                   (!palette || n_colors > 0),
               "%s: a palette or counts need 1..%d colours, got %d", fn, RN_MAXCOL, n_colors);
  VR_CHECK_ARG(!class_map || mix_type == 2 || palette, "%s: mix_type %d of a class map needs a palette", fn, mix_type);
  VR_CHECK_ARG(class_map || !counts, "%s: counts need a class map", fn);
  return VR_OK;
}

}  // namespace

extern "C" int vrnet_render_u8(const unsigned char* frames, const unsigned char* class_map, int B, int ih, int iw,
                               const unsigned char* palette, int n_colors, int mix_type, float alpha, const int* boxes,
                               const int* box_offsets, int n_rows, const unsigned char* box_palette, int n_box_colors,
                               int thickness, unsigned char* out, long long* counts, int* flag, void* stream) {
  if (const int rc = render_check("render", frames && out, "frames", B, ih, iw, class_map, palette, n_colors, mix_type, alpha,
                                  counts))
    return rc;
  VR_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || (boxes && box_offsets && box_palette && n_box_colors > 0 &&
                                                n_box_colors <= RN_MAXCOL && thickness > 0 && thickness <= (1 << 24))),
               "render: %d box rows need offsets, a box palette of 1..%d colours and 0 < thickness <= 2^24", n_rows, RN_MAXCOL);
  const long total = (long)B * ih * iw;
  const bool same = out == frames;
  VR_CHECK_ARG(same ? class_map == nullptr : !overlap(out, 3 * total, frames, 3 * total),
               "render: out may be the frames themselves when there is no class map, and must not overlap them otherwise");
  VR_CHECK_ARG(!class_map || !overlap(out, 3 * total, class_map, total), "render: out overlaps the class map");
  hipStream_t st = vr_stream(stream);
  if (counts && hipMemsetAsync(counts, 0, (size_t)B * n_colors * sizeof(long long), st) != hipSuccess) {
    vr_set_error("render: clearing the counts failed");
    return VR_ERR_LAUNCH;
  }
  if (same && n_rows == 0) return VR_OK;            // boxes in place, and there are none
  RenderArgs p{};
  p.frames = frames; p.cmap = class_map; p.palette = palette; p.out = out;
  p.boxes = n_rows > 0 ? boxes : nullptr; p.offsets = box_offsets; p.box_palette = box_palette;
  p.counts = reinterpret_cast<unsigned long long*>(counts); p.flag = flag;
  p.B = B; p.ih = ih; p.iw = iw; p.n_colors = n_colors; p.n_box_colors = n_box_colors; p.n_rows = n_rows;
  p.thickness = thickness; p.mix = mix_type; p.alpha = alpha; p.inplace = same; p.total = (int)total;
  // dword accesses need frames + 3 h, out + 3 h and class_map + h on 4-byte boundaries for one head h of 0..3 pixels:
  // 3 h = -f (mod 4) gives h = f (mod 4)
  const int h = (int)(reinterpret_cast<uintptr_t>(frames) & 3);
  p.vec = (reinterpret_cast<uintptr_t>(out) & 3) == (uintptr_t)h &&
          (!class_map || ((reinterpret_cast<uintptr_t>(class_map) + h) & 3) == 0);
  p.head = p.vec ? (int)(h < total ? h : total) : 0;
  p.ngroups = (int)((total - p.head) / 4);
  long grid = vr_cdiv(p.ngroups, 256);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)grid), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("render");
  return VR_OK;
}

extern "C" int vrnet_render_ragged_u8(const unsigned char* frames, const unsigned char* class_map,
                                      const vrnet_frame_geom* geom, int B, int ihm, int iwm, const unsigned char* palette,
                                      int n_colors, int mix_type, float alpha, const int* boxes, const int* box_offsets,
                                      int n_rows, const unsigned char* box_palette, int n_box_colors, unsigned char* out,
                                      long long* counts, int* flag, void* stream) {
  if (const int rc = render_check("render_ragged", frames && out && geom && B < 65536, "slots", B, ihm, iwm, class_map, palette,
                                  n_colors, mix_type, alpha, counts))
    return rc;
  VR_CHECK_ARG(n_rows >= 0 && (n_rows == 0 || (boxes && box_offsets && box_palette && n_box_colors > 0 &&
                                                n_box_colors <= RN_MAXCOL)),
               "render_ragged: %d box rows need offsets and a box palette of 1..%d colours", n_rows, RN_MAXCOL);
  const long total = (long)B * ihm * iwm;
  VR_CHECK_ARG(!overlap(out, 3 * total, frames, 3 * total), "render_ragged: out overlaps the frames (the padding is written)");
  VR_CHECK_ARG(!class_map || !overlap(out, 3 * total, class_map, total), "render_ragged: out overlaps the class map");
  hipStream_t st = vr_stream(stream);
  if (counts && hipMemsetAsync(counts, 0, (size_t)B * n_colors * sizeof(long long), st) != hipSuccess) {
    vr_set_error("render_ragged: clearing the counts failed");
    return VR_ERR_LAUNCH;
  }
  RaggedRenderArgs a{};
  RenderArgs& p = a.r;
  a.tab = geom;
  p.frames = frames; p.cmap = class_map; p.palette = palette; p.out = out;
  p.boxes = n_rows > 0 ? boxes : nullptr; p.offsets = box_offsets; p.box_palette = box_palette;
  p.counts = reinterpret_cast<unsigned long long*>(counts); p.flag = flag;
  p.B = B; p.ih = ihm; p.iw = iwm; p.n_colors = n_colors; p.n_box_colors = n_box_colors; p.n_rows = n_rows;
  p.mix = mix_type; p.alpha = alpha;
  // dword accesses: every slot starts on a 4-byte boundary in all three tensors
  const long slot = (long)ihm * iwm;
  p.vec = ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(class_map)) & 3) == 0 &&
          (slot % 4 == 0 || B == 1);
  long grid = vr_cdiv(vr_cdiv(slot, 4), 256);
  const long per_image = vr_cdiv(2048, B);
  if (grid > per_image) grid = per_image;
  hipLaunchKernelGGL(render_ragged_kernel, dim3((unsigned)grid, B), dim3(256), 0, st, a);
  VR_LAUNCH_CHECK("render_ragged");
  return VR_OK;
}
