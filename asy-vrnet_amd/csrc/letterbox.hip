// The letterbox in front of the network, on the device and from raw bytes: utils/utils.py:19-32 and utils_seg/utils.py:19-31
// `resize_image` (detect_image, get_FPS, get_map_txt, both EvalCallbacks) and the `random=False` branch of get_random_data
// (utils/dataloader.py:131-146) -- Pillow's Image.resize(BICUBIC) of the frame pasted on a grey (128) canvas, and
// Image.resize(NEAREST) of the label map pasted on a 0 canvas.  Pillow's 8-bit resample (Resample.c ImagingResample) is
// integer arithmetic on 22-bit fixed-point coefficients, two separable passes with a rounded, clipped uint8 image between
// them; its nearest resize (Geometry.c ImagingScaleAffine) is a running double sum per axis.  Both are reproduced here
// BIT FOR BIT: the outputs equal Pillow's bytes, not merely approximate them.
//   tables      the coefficient tables, built on the device in double with one rounding per operation (contract off), so
//               a call needs no host table, no copy and no synchronisation: one thread per output column / row computes
//               its window (xmin, n) and its n integer taps (weights summed, then recomputed and normalised: no
//               per-thread array); one thread per axis runs the nearest-neighbour recurrence, which is sequential
//   horizontal  (B, ih, iw, 3) -> uint8 (B, ih, nw, 3) in the workspace, one thread per output pixel; skipped when
//               nw == iw, as Pillow skips it
//   vertical    one thread per CANVAS pixel: the vertical taps over the horizontal result (a copy when nh == ih), the
//               paste at (dx, dy), the padding, the normalisation of batch_formats_kernel (double, rounded once) and the
//               stores -- canvas rows, CHW planes and the label canvas, each coalesced over a wave's consecutive x
// The accumulator is int32 as Pillow's: the taps of a row are normalised to sum 1 with negative lobes, sum |k| < 1.4 * 2^22
// for the bicubic kernel at any scale, so |2^21 + sum k * v| < 2^21 + 255 * 1.4 * 2^22 < 1.5e9 < 2^31.
#include "resample.h"               // bicubic_taps, resample_taps3, normalise_store, lb_ksize: shared with augment.hip, mosaic.hip

#pragma clang fp contract(off)

namespace {

struct LetterboxArgs {
  const unsigned char* img;          // (B, ih, iw, 3)
  const unsigned char* label;        // (B, ih, iw) or null
  int B, ih, iw, H, W, nw, nh, dx, dy;
  int ksh, ksv;                      // tap capacity of a column / row table entry
  int *hb, *hk, *vb, *vk;            // bounds (xmin, n) per output index; taps, tap-major: k[t * out + index]
  int *xi, *yi;                      // nearest-neighbour source index per window column / row
  unsigned char* mid;                // (B, ih, nw, 3): the horizontal pass's result
  unsigned char* canvas;             // (B, H, W, 3) or null
  float* images;                     // (B, 3, H, W) or null
  unsigned char* label_out;          // (B, H, W) or null
};

__global__ __launch_bounds__(256) void letterbox_tables_kernel(const LetterboxArgs p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool pixels = p.canvas || p.images;
  if (e < p.nw) {
    if (pixels && p.nw != p.iw) bicubic_taps(e, p.iw, p.nw, p.ksh, p.hb, p.hk);
  } else if (e < p.nw + p.nh) {
    if (pixels && p.nh != p.ih) bicubic_taps(e - p.nw, p.ih, p.nh, p.ksv, p.vb, p.vk);
  } else if (p.label_out) {
    if (e == p.nw + p.nh) vr_nearest_indices(p.iw, p.nw, p.xi);
    if (e == p.nw + p.nh + 1) vr_nearest_indices(p.ih, p.nh, p.yi);
  }
}

__global__ __launch_bounds__(256) void letterbox_horizontal_kernel(const LetterboxArgs p) {
  const long total = (long)p.B * p.ih * p.nw;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long row = e / p.nw;
  const int xx = (int)(e - row * p.nw);
  const int xmin = p.hb[2 * xx], n = p.hb[2 * xx + 1];
  const unsigned char* src = p.img + (row * p.iw + xmin) * 3;
  resample_taps3(src, 3, p.hk + xx, p.nw, n, p.mid + e * 3);
}

__global__ __launch_bounds__(256) void letterbox_vertical_paste_kernel(const LetterboxArgs p) {
  const long HW = (long)p.H * p.W;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.B * HW) return;
  const long b = e / HW, r = e - b * HW;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const int wx = x - p.dx, wy = y - p.dy;
  const bool inside = wx >= 0 && wx < p.nw && wy >= 0 && wy < p.nh;
  unsigned char v[3] = {128, 128, 128};
  if (inside && (p.canvas || p.images)) {
    // the horizontal result: the workspace, or the frame itself when that pass was skipped (then nw == iw)
    const unsigned char* src = (p.nw != p.iw ? p.mid : p.img) + (b * p.ih * p.nw + wx) * 3;
    const long rs = (long)p.nw * 3;
    if (p.nh != p.ih) {
      const int ymin = p.vb[2 * wy], n = p.vb[2 * wy + 1];
      resample_taps3(src + ymin * rs, rs, p.vk + wy, p.nh, n, v);
    } else {
      src += wy * rs;
      v[0] = src[0];
      v[1] = src[1];
      v[2] = src[2];
    }
  }
  if (p.canvas) {
    p.canvas[e * 3] = v[0];
    p.canvas[e * 3 + 1] = v[1];
    p.canvas[e * 3 + 2] = v[2];
  }
  if (p.images) normalise_store(p.images, b, HW, r, v);
  if (p.label_out) {
    unsigned char lab = 0;
    if (inside) {
      const int sx = p.xi[wx], sy = p.yi[wy];
      if (sx < p.iw && sy < p.ih) lab = p.label[(b * p.ih + sy) * p.iw + sx];   // ImagingScaleAffine leaves the rest unset
    }
    p.label_out[e] = lab;
  }
}

long lb_table_ints(int ih, int iw, int nh, int nw) {
  return (long)nw * (2 + lb_ksize(iw, nw) + 1) + (long)nh * (2 + lb_ksize(ih, nh) + 1);
}

// ---- the ragged form: frames of their own sizes in the corners of (ihm, iwm) slots, the geometry of image b in tab[b].
// The same arithmetic (bicubic_taps, nearest_indices, clip8, normalise_store); the tables of image b live in slot b of the
// workspace, sized by the canvas and the caller's tap capacity; blockIdx.y is the image, so a block reads one record.
struct RaggedLetterboxArgs {
  const unsigned char* img;          // (B, ihm, iwm, 3)
  const unsigned char* label;        // (B, ihm, iwm) or null
  const vrnet_frame_geom* tab;       // (B)
  int B, ihm, iwm, H, W, cap;        // cap: taps per table entry
  long slot;                         // ints of one image's tables
  int* tables;
  unsigned char* mid;                // (B, ihm, W, 3): the horizontal pass's result, rows of W pixels
  unsigned char* canvas;             // (B, H, W, 3) or null
  float* images;                     // (B, 3, H, W) or null
  unsigned char* label_out;          // (B, H, W) or null
  int* flag;                         // or null
};

struct RaggedTables {
  int *hb, *hk, *vb, *vk, *xi, *yi;
};

__device__ __forceinline__ RaggedTables ragged_tables(const RaggedLetterboxArgs& p, int b) {
  RaggedTables s;
  int* t = p.tables + b * p.slot;
  s.hb = t; t += 2L * p.W;
  s.hk = t; t += (long)p.W * p.cap;
  s.vb = t; t += 2L * p.H;
  s.vk = t; t += (long)p.H * p.cap;
  s.xi = t; t += p.W;
  s.yi = t;
  return s;
}

// the record of this block's image; an image or window without pixels is `empty`: its canvas is all padding
__device__ __forceinline__ vrnet_frame_geom ragged_geom(const RaggedLetterboxArgs& p, int b, bool& empty, bool& bad) {
  const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  empty = g.ih <= 0 || g.iw <= 0 || g.nw <= 0 || g.nh <= 0;
  return g;
}

__global__ __launch_bounds__(256) void letterbox_ragged_tables_kernel(const RaggedLetterboxArgs p) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  bool empty, bad;
  const vrnet_frame_geom g = ragged_geom(p, b, empty, bad);
  const bool pixels = p.canvas || p.images;
  if (e == 0 && p.flag) {            // a clamped record, or taps beyond the slot's capacity (bicubic_taps then truncates them)
    if (!empty && pixels)
      bad = bad || (g.nw != g.iw && lb_ksize(g.iw, g.nw) > p.cap) || (g.nh != g.ih && lb_ksize(g.ih, g.nh) > p.cap);
    if (bad) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  }
  if (empty) return;
  const RaggedTables s = ragged_tables(p, b);
  if (e < p.W) {
    if (e < g.nw && pixels && g.nw != g.iw) bicubic_taps(e, g.iw, g.nw, p.cap, s.hb, s.hk);
  } else if (e < p.W + p.H) {
    const int y = e - p.W;
    if (y < g.nh && pixels && g.nh != g.ih) bicubic_taps(y, g.ih, g.nh, p.cap, s.vb, s.vk);
  } else if (p.label_out) {
    if (e == p.W + p.H) vr_nearest_indices(g.iw, g.nw, s.xi);
    if (e == p.W + p.H + 1) vr_nearest_indices(g.ih, g.nh, s.yi);
  }
}

__global__ __launch_bounds__(256) void letterbox_ragged_horizontal_kernel(const RaggedLetterboxArgs p) {
  const int b = blockIdx.y;
  bool empty, bad;
  const vrnet_frame_geom g = ragged_geom(p, b, empty, bad);
  if (empty || g.nw == g.iw) return;             // this image skips the pass, as Pillow does
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(e / p.W), xx = (int)(e - (long)row * p.W);
  if (row >= g.ih || xx >= g.nw) return;
  const RaggedTables s = ragged_tables(p, b);
  const int xmin = s.hb[2 * xx], n = s.hb[2 * xx + 1];
  const unsigned char* src = p.img + (((long)b * p.ihm + row) * p.iwm + xmin) * 3;
  resample_taps3(src, 3, s.hk + xx, g.nw, n, p.mid + (((long)b * p.ihm + row) * p.W + xx) * 3);
}

__global__ __launch_bounds__(256) void letterbox_ragged_vertical_paste_kernel(const RaggedLetterboxArgs p) {
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= HW) return;
  bool empty, bad;
  const vrnet_frame_geom g = ragged_geom(p, (int)b, empty, bad);
  const RaggedTables s = ragged_tables(p, (int)b);
  const long e = b * HW + r;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const int wx = x - g.dx, wy = y - g.dy;
  const bool inside = !empty && wx >= 0 && wx < g.nw && wy >= 0 && wy < g.nh;
  unsigned char v[3] = {128, 128, 128};
  if (inside && (p.canvas || p.images)) {
    // the horizontal result: the workspace (rows of W pixels), or the frame's own slot when that pass was skipped
    const bool resized = g.nw != g.iw;
    const unsigned char* src = resized ? p.mid + (b * p.ihm * p.W + wx) * 3 : p.img + (b * p.ihm * p.iwm + wx) * 3;
    const long rs = (resized ? (long)p.W : (long)p.iwm) * 3;
    if (g.nh != g.ih) {
      const int ymin = s.vb[2 * wy], n = s.vb[2 * wy + 1];
      resample_taps3(src + ymin * rs, rs, s.vk + wy, g.nh, n, v);
    } else {
      src += wy * rs;
      v[0] = src[0];
      v[1] = src[1];
      v[2] = src[2];
    }
  }
  if (p.canvas) {
    p.canvas[e * 3] = v[0];
    p.canvas[e * 3 + 1] = v[1];
    p.canvas[e * 3 + 2] = v[2];
  }
  if (p.images) normalise_store(p.images, b, HW, r, v);
  if (p.label_out) {
    unsigned char lab = 0;
    if (inside) {
      const int sx = s.xi[wx], sy = s.yi[wy];
      if (sx >= 0 && sx < g.iw && sy >= 0 && sy < g.ih) lab = p.label[(b * p.ihm + sy) * p.iwm + sx];
    }
    p.label_out[e] = lab;
  }
}

}  // namespace

extern "C" long vrnet_letterbox_workspace(int B, int ih, int iw, int nh, int nw) {
  if (B <= 0 || ih <= 0 || iw <= 0 || nh <= 0 || nw <= 0) return 0;
  return lb_align(lb_table_ints(ih, iw, nh, nw) * (long)sizeof(int)) + (nw != iw ? lb_align((long)B * ih * nw * 3) : 0);
}

extern "C" int vrnet_letterbox_u8(const unsigned char* img, const unsigned char* label, int B, int ih, int iw, int H, int W,
                                  int nw, int nh, int dx, int dy, unsigned char* canvas, float* images,
                                  unsigned char* label_out, void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(B > 0 && ih > 0 && iw > 0 && H > 0 && W > 0, "letterbox: bad shape (B %d, frame %d x %d, canvas %d x %d)", B, ih,
               iw, H, W);
  VR_CHECK_ARG(nw > 0 && nw <= W && nh > 0 && nh <= H, "letterbox: the window %d x %d must be non-empty and fit the %d x %d canvas",
               nh, nw, H, W);
  VR_CHECK_ARG(dx >= 0 && dy >= 0 && (long)dx + nw <= W && (long)dy + nh <= H,
               "letterbox: the window %d x %d at (%d, %d) must lie inside the %d x %d canvas", nh, nw, dy, dx, H, W);
  VR_CHECK_ARG(canvas || images || label_out, "letterbox: no output requested");
  VR_CHECK_ARG(img || !(canvas || images), "letterbox: an image output needs the frames");
  VR_CHECK_ARG(label || !label_out, "letterbox: a label output needs the label maps");
  VR_CHECK_ARG((long)B * ih * iw < (1L << 40) && (long)B * H * W < (1L << 39), "letterbox: batch too large");
  const long need = vrnet_letterbox_workspace(B, ih, iw, nh, nw);
  if (!workspace || workspace_bytes < need) {
    vr_set_error("letterbox: workspace %ld < %ld bytes", workspace ? workspace_bytes : 0L, need);
    return VR_ERR_WORKSPACE;
  }
  LetterboxArgs p{};
  p.img = img; p.label = label;
  p.B = B; p.ih = ih; p.iw = iw; p.H = H; p.W = W; p.nw = nw; p.nh = nh; p.dx = dx; p.dy = dy;
  p.ksh = lb_ksize(iw, nw);
  p.ksv = lb_ksize(ih, nh);
  int* t = static_cast<int*>(workspace);
  p.hb = t; t += 2L * nw;
  p.hk = t; t += (long)nw * p.ksh;
  p.vb = t; t += 2L * nh;
  p.vk = t; t += (long)nh * p.ksv;
  p.xi = t; t += nw;
  p.yi = t;
  p.mid = static_cast<unsigned char*>(workspace) + lb_align(lb_table_ints(ih, iw, nh, nw) * (long)sizeof(int));
  p.canvas = canvas; p.images = images; p.label_out = label_out;
  hipStream_t st = vr_stream(stream);
  const bool pixels = canvas || images;
  hipLaunchKernelGGL(letterbox_tables_kernel, dim3((unsigned)vr_cdiv((long)nw + nh + 2, 256)), dim3(256), 0, st, p);
  if (pixels && nw != iw)
    hipLaunchKernelGGL(letterbox_horizontal_kernel, dim3((unsigned)vr_cdiv((long)B * ih * nw, 256)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(letterbox_vertical_paste_kernel, dim3((unsigned)vr_cdiv((long)B * H * W, 256)), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("letterbox");
  return VR_OK;
}

extern "C" long vrnet_letterbox_ragged_workspace(int B, int ihm, int iwm, int H, int W, int max_taps) {
  if (B <= 0 || ihm <= 0 || iwm <= 0 || H <= 0 || W <= 0 || max_taps <= 0) return 0;
  return lb_align(B * lb_ragged_slot_ints(H, W, max_taps) * (long)sizeof(int)) + lb_align((long)B * ihm * W * 3);
}

extern "C" int vrnet_letterbox_ragged_u8(const unsigned char* img, const unsigned char* label, const vrnet_frame_geom* geom,
                                         int B, int ihm, int iwm, int H, int W, int max_taps, unsigned char* canvas,
                                         float* images, unsigned char* label_out, int* flag, void* workspace,
                                         long workspace_bytes, void* stream) {
  VR_CHECK_ARG(geom && B > 0 && B < 65536 && ihm > 0 && iwm > 0 && H > 0 && W > 0 && max_taps >= 5 && max_taps <= 4096,
               "letterbox_ragged: bad shape (B %d, slots %d x %d, canvas %d x %d, max_taps %d)", B, ihm, iwm, H, W, max_taps);
  VR_CHECK_ARG(canvas || images || label_out, "letterbox_ragged: no output requested");
  VR_CHECK_ARG(img || !(canvas || images), "letterbox_ragged: an image output needs the frames");
  VR_CHECK_ARG(label || !label_out, "letterbox_ragged: a label output needs the label maps");
  VR_CHECK_ARG((long)B * ihm * iwm < (1L << 31) && (long)B * H * W < (1L << 31) && (long)B * ihm * W < (1L << 31) &&
                   (long)B * lb_ragged_slot_ints(H, W, max_taps) < (1L << 31),
               "letterbox_ragged: batch too large");
  const long need = vrnet_letterbox_ragged_workspace(B, ihm, iwm, H, W, max_taps);
  if (!workspace || workspace_bytes < need) {
    vr_set_error("letterbox_ragged: workspace %ld < %ld bytes", workspace ? workspace_bytes : 0L, need);
    return VR_ERR_WORKSPACE;
  }
  RaggedLetterboxArgs p{};
  p.img = img; p.label = label; p.tab = geom;
  p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.cap = max_taps;
  p.slot = lb_ragged_slot_ints(H, W, max_taps);
  p.tables = static_cast<int*>(workspace);
  p.mid = static_cast<unsigned char*>(workspace) + lb_align(B * p.slot * (long)sizeof(int));
  p.canvas = canvas; p.images = images; p.label_out = label_out; p.flag = flag;
  hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(letterbox_ragged_tables_kernel, dim3((unsigned)vr_cdiv((long)W + H + 2, 256), B), dim3(256), 0, st, p);
  if (canvas || images)
    hipLaunchKernelGGL(letterbox_ragged_horizontal_kernel, dim3((unsigned)vr_cdiv((long)ihm * W, 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(letterbox_ragged_vertical_paste_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("letterbox_ragged");
  return VR_OK;
}
