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
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int LB_PRECISION_BITS = 32 - 8 - 2;      // Resample.c PRECISION_BITS

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

// Resample.c bicubic_filter, a = -0.5
__device__ __forceinline__ double bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// Resample.c precompute_coeffs + normalize_coeffs_8bpc for output index xx of an axis resized in -> out
__device__ void bicubic_taps(int xx, int in, int out, int cap, int* bounds, int* k) {
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  int n = xmax - xmin;
  if (n > cap) n = cap;              // never taken: n <= 2 * support + 1 <= cap; keeps the stores inside the table
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < n; ++x) {
    double w = bicubic((x + xmin - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[(long)x * out + xx] = w < 0 ? (int)(-0.5 + w * (1 << LB_PRECISION_BITS)) : (int)(0.5 + w * (1 << LB_PRECISION_BITS));
  }
  bounds[2 * xx] = xmin;
  bounds[2 * xx + 1] = n;
}

// Geometry.c ImagingScaleAffine: the source index of each output index, a running sum (not x * a0)
__device__ void nearest_indices(int in, int out, int* idx) {
  const double a0 = (double)in / out;
  double xo = a0 * 0.5;
  for (int x = 0; x < out; ++x) {
    idx[x] = (int)xo;
    xo += a0;
  }
}

__global__ __launch_bounds__(256) void letterbox_tables_kernel(const LetterboxArgs p) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool pixels = p.canvas || p.images;
  if (e < p.nw) {
    if (pixels && p.nw != p.iw) bicubic_taps(e, p.iw, p.nw, p.ksh, p.hb, p.hk);
  } else if (e < p.nw + p.nh) {
    if (pixels && p.nh != p.ih) bicubic_taps(e - p.nw, p.ih, p.nh, p.ksv, p.vb, p.vk);
  } else if (p.label_out) {
    if (e == p.nw + p.nh) nearest_indices(p.iw, p.nw, p.xi);
    if (e == p.nw + p.nh + 1) nearest_indices(p.ih, p.nh, p.yi);
  }
}

__device__ __forceinline__ unsigned char clip8(int acc) {
  acc >>= LB_PRECISION_BITS;
  return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

__global__ __launch_bounds__(256) void letterbox_horizontal_kernel(const LetterboxArgs p) {
  const long total = (long)p.B * p.ih * p.nw;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long row = e / p.nw;
  const int xx = (int)(e - row * p.nw);
  const int xmin = p.hb[2 * xx], n = p.hb[2 * xx + 1];
  const unsigned char* src = p.img + (row * p.iw + xmin) * 3;
  const int* k = p.hk + xx;
  int a0 = 1 << (LB_PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < n; ++t) {
    const int w = k[(long)t * p.nw];
    a0 += w * src[3 * t];
    a1 += w * src[3 * t + 1];
    a2 += w * src[3 * t + 2];
  }
  unsigned char* dst = p.mid + e * 3;
  dst[0] = clip8(a0);
  dst[1] = clip8(a1);
  dst[2] = clip8(a2);
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
      const int* k = p.vk + wy;
      src += ymin * rs;
      int a0 = 1 << (LB_PRECISION_BITS - 1), a1 = a0, a2 = a0;
      for (int t = 0; t < n; ++t) {
        const int w = k[(long)t * p.nh];
        a0 += w * src[t * rs];
        a1 += w * src[t * rs + 1];
        a2 += w * src[t * rs + 2];
      }
      v[0] = clip8(a0);
      v[1] = clip8(a1);
      v[2] = clip8(a2);
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
  if (p.images) {                    // batch_formats_kernel's arithmetic: ((v / 255) - mean) / std in double, rounded once
    const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double d = (double)v[c];
      d /= 255.0;
      d -= mean[c];
      d /= sd[c];
      p.images[(b * 3 + c) * HW + r] = (float)d;
    }
  }
  if (p.label_out) {
    unsigned char lab = 0;
    if (inside) {
      const int sx = p.xi[wx], sy = p.yi[wy];
      if (sx < p.iw && sy < p.ih) lab = p.label[(b * p.ih + sy) * p.iw + sx];   // ImagingScaleAffine leaves the rest unset
    }
    p.label_out[e] = lab;
  }
}

// Resample.c precompute_coeffs: ksize, the tap capacity of one output index
int lb_ksize(int in, int out) {
  double fs = (double)in / out;
  if (fs < 1.0) fs = 1.0;
  return (int)ceil(2.0 * fs) * 2 + 1;
}

long lb_table_ints(int ih, int iw, int nh, int nw) {
  return (long)nw * (2 + lb_ksize(iw, nw) + 1) + (long)nh * (2 + lb_ksize(ih, nh) + 1);
}

long lb_align(long n) { return (n + 255) / 256 * 256; }

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
