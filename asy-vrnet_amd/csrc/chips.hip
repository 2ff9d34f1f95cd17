// Fixed-size detection chips: every kept detection cut out of the ORIGINAL frame as csrc/crops.hip cuts it and brought to one
// size (sh, sw) with Pillow's 8-bit BICUBIC, the way the reference brings any picture to a fixed size (resize_image,
// utils/utils.py:19-32) -- one tensor of equal-sized pictures for a second stage.
//
// THE RULE (host statement, with Pillow itself: render.chip_boxes_host and render.chip_geometry).  Row n = left, top, right,
// bottom, class of image b is clamped as vrnet_crop_boxes_u8 clamps it: l, t, w = r - l, h = bt - t.  w <= 0 or h <= 0: the
// chip is all grey 128 (state 2).  letterbox == 0: the chip is image.crop((l, t, r, bt)).resize((sw, sh), BICUBIC) -- crop THEN
// resize, the taps stop at the crop's edge.  letterbox != 0: scale = min(sw / w, sh / h) in doubles, nw = max(int(w scale), 1),
// nh = max(int(h scale), 1) (the max is this project's: the reference lets Pillow raise on a 1000 x 3 crop), the crop resized
// to (nw, nh) and pasted at ((sw - nw) / 2, (sh - nh) / 2) on grey 128.
//
// THE ARITHMETIC is Resample.c's, from resample.h: per output index xx of an axis in -> out the window (xmin, n) and the sum
// ww of its n bicubic values in the order x = 0 .. n - 1; the integer weight of tap x is bicubic((x + xmin - center + 0.5) ss)
// / ww rounded to 22 bits, which any thread can recompute from (xmin, n, ww) -- so the table is 16 bytes an index whatever the
// scale, and there is no tap capacity.  Each pass sums w * byte in int32 on top of 1 << 21; integer addition is associative,
// so the source rows may be streamed in chunks.  The one ordering Pillow imposes is the rounding to bytes between the
// horizontal and the vertical pass, and it is kept: the horizontal pass of a chunk goes into LDS as bytes.  A pass whose size
// does not change has the weights (0, 1, 0, 0) exactly and is the identity, as Pillow's skipped pass is.
//
// TWO LAUNCHES, both grids from n_cap, sh and sw alone.  chip_tables_kernel, one workgroup per row of the table: the image
// of the row (the first offset above n, which is the offsets made monotone as crop_layout_kernel makes them), the clamp, the
// geometry, the record, and one thread per output index of each axis for (xmin, n, ww).  chip_resample_kernel, one workgroup
// per (row, band of CH_BAND chip rows): it streams the source rows [ymin(first), ymax(last)) of its band in chunks of CH_CHUNK
// -- horizontal pass into LDS, then every chunk row is added into the int32 accumulators (registers: thread t owns the bytes
// t, t + 256, t + 512 of each of the band's chip rows) of the chip rows whose window holds it -- and at the end clips, pastes,
// fills the grey border and writes the float form through normalise_store.  LDS is bounded by the chunk, not by the crop: the
// horizontal weights are kept in LDS where all of them fit and recomputed per tap where they do not, the same integers.  A
// workgroup behind the last row leaves at once and writes nothing; one of an empty row writes grey.  It trusts the tables
// for (xmin, n, ww) alone and clamps the window to the crop: l, t, w, h and the geometry are derived again from the row.
#include "resample.h"

#include <climits>

namespace {

constexpr int CH_BAND = 8;           // chip rows per workgroup of the resample launch
constexpr int CH_CHUNK = 16;         // source rows per pass through LDS
constexpr int CH_MAX = 256;          // the largest side of a chip: 3 CH_MAX bytes a row = three per thread
constexpr int CH_PER = 3 * CH_MAX / 256;
constexpr int CH_WCACHE = 4096;      // horizontal weights kept in LDS; more than that are recomputed per tap

struct ChipAxis {                    // one output index of one axis
  int xmin, n;
  double ww;
};                                   // 16 bytes

struct ChipArgs {
  const unsigned char* frames;       // (B, ihm, iwm, 3)
  const vrnet_frame_geom* geom;      // (B) or NULL: every image is ihm x iwm
  const int* rows;                   // (n_cap, 5)
  const int* offsets;                // (B + 1)
  unsigned char* chips;              // (n_cap, sh, sw, 3)
  float* chips_f32;                  // (n_cap, 3, sh, sw) or NULL
  vrnet_chip_rec* table;             // (n_cap)
  int* summary;                      // (1)
  ChipAxis* axes;                    // (n_cap, sw + sh): the columns, then the rows
  int* flag;
  int B, ihm, iwm, n_cap, sh, sw, letterbox;
};

// the clamp of a row to its image (crop_window of crops.hip): x, y = l, t; z, w = w, h (both 0 for an empty crop)
__device__ __forceinline__ int4 chip_window(const int* row, int ih, int iw) {
  const int l = vr_clampi(row[0], 0, iw), t = vr_clampi(row[1], 0, ih);
  const int r = vr_clampi(row[2], 0, iw), bt = vr_clampi(row[3], 0, ih);
  const int w = r - l, h = bt - t;
  return (w <= 0 || h <= 0) ? make_int4(l, t, 0, 0) : make_int4(l, t, w, h);
}

// render.chip_geometry for a non-empty crop: x, y = nw, nh; z, w = dx, dy.  resize_image's doubles, each operation rounded once
__device__ __forceinline__ int4 chip_geometry(int w, int h, int sh, int sw, int letterbox) {
  if (!letterbox) return make_int4(sw, sh, 0, 0);
  const double sx = (double)sw / (double)w, sy = (double)sh / (double)h;
  const double scale = sy < sx ? sy : sx;
  // w scale <= sw (1 + 2^-52)^2 < sw + 1, so the upper clamp never acts; it is there for the stores
  const int nw = vr_clampi((int)((double)w * scale), 1, sw), nh = vr_clampi((int)((double)h * scale), 1, sh);
  return make_int4(nw, nh, (sw - nw) / 2, (sh - nh) / 2);
}

// Resample.c precompute_coeffs for output index xx of an axis in -> out: the window and the sum of its bicubic values
__device__ inline ChipAxis chip_axis(int xx, int in, int out) {
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in) xmax = in;
  const int n = xmax - xmin;
  double ww = 0.0;
  for (int x = 0; x < n; ++x) ww += bicubic((x + xmin - center + 0.5) * ss);
  return ChipAxis{xmin, n, ww};
}

// what every tap of output index xx shares, and normalize_coeffs_8bpc for tap x of it
struct ChipTaps {
  double center, ss, ww;
  int xmin, n;
};
__device__ __forceinline__ ChipTaps chip_taps(const ChipAxis a, int xx, int in, int out) {
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  ChipTaps k;
  k.center = (xx + 0.5) * scale;
  k.ss = 1.0 / fs;
  k.ww = a.ww;
  k.xmin = vr_clampi(a.xmin, 0, in);               // whatever the table holds, no tap leaves the crop
  k.n = vr_clampi(a.n, 0, in - k.xmin);
  return k;
}
__device__ __forceinline__ int chip_weight(const ChipTaps& k, int x) {
  double w = bicubic((x + k.xmin - k.center + 0.5) * k.ss);
  if (k.ww != 0.0) w /= k.ww;
  return w < 0 ? (int)(-0.5 + w * (1 << LB_PRECISION_BITS)) : (int)(0.5 + w * (1 << LB_PRECISION_BITS));
}

__global__ __launch_bounds__(256) void chip_tables_kernel(const ChipArgs p) {
  __shared__ int s_image;
  const int n = blockIdx.x, tid = threadIdx.x;      // the workgroup's row: everything but the axis loop is wave-uniform
  const int N = vr_clampi(p.offsets[p.B], 0, p.n_cap);
  if (n == 0 && tid == 0) p.summary[0] = N;
  if (n >= N) {                                     // behind the last row, whatever the row holds
    if (tid == 0) p.table[n] = vrnet_chip_rec{-1, 0, 0, 0, 0, 0, 0, 0};
    return;
  }
  if (tid < 64) {                                   // the first offset above n: n < N <= offsets[B], so there is one
    int first = p.B;
    for (int j0 = 0; j0 <= p.B; j0 += 64) {
      const int j = j0 + tid;
      const unsigned long long hit = __ballot(j <= p.B && p.offsets[j] > n);
      if (hit) {
        first = j0 + __ffsll(hit) - 1;
        break;
      }
    }
    if (tid == 0) s_image = max(first, 1) - 1;      // c[0] = 0: offsets[0] > n still means image 0
  }
  __syncthreads();
  const int b = s_image;
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, b, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
  const int4 q = chip_window(p.rows + 5L * n, ih, iw);
  if (tid == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  if (q.z == 0) {
    if (tid == 0) p.table[n] = vrnet_chip_rec{b, 0, 0, 0, 0, 0, 0, 2};
    return;
  }
  const int4 g = chip_geometry(q.z, q.w, p.sh, p.sw, p.letterbox);
  if (tid == 0) p.table[n] = vrnet_chip_rec{b, q.z, q.w, g.x, g.y, g.z, g.w, 1};
  ChipAxis* axes = p.axes + (long)n * (p.sw + p.sh);
  for (int i = tid; i < g.x + g.y; i += 256) {
    if (i < g.x) axes[i] = chip_axis(i, q.z, g.x);
    else axes[p.sw + i - g.x] = chip_axis(i - g.x, q.w, g.y);
  }
}

__global__ __launch_bounds__(256) void chip_resample_kernel(const ChipArgs p, int bands) {
  __shared__ unsigned char s_mid[CH_CHUNK * 3 * CH_MAX];       // the horizontal pass of a chunk; then the band's chip bytes
  __shared__ int s_wv[CH_CHUNK * CH_BAND];                     // the vertical weight of chunk row r for chip row k of the band
  __shared__ int s_wh[CH_WCACHE];                              // the horizontal weights, tap x of index xx at x nw + xx
  const int n = blockIdx.x / bands, band = blockIdx.x % bands, tid = threadIdx.x;
  const vrnet_chip_rec rec = p.table[n];
  if (rec.state == 0 || rec.image < 0 || rec.image >= p.B) return;          // behind the last row: nothing is written
  int ih, iw;
  bool bad;
  vr_image_size(p.geom, rec.image, p.ihm, p.iwm, p.ihm, p.iwm, ih, iw, bad);
  const int4 q = chip_window(p.rows + 5L * n, ih, iw);
  const int w = q.z, h = q.w, sh = p.sh, sw = p.sw;
  const int4 g = w > 0 ? chip_geometry(w, h, sh, sw, p.letterbox) : make_int4(0, 0, 0, 0);
  const int nw = g.x, nh = g.y, dx = g.z, dy = g.w;
  const int Y0 = band * CH_BAND, rows_here = min(CH_BAND, sh - Y0), D = 3 * sw, Dm = 3 * nw;
  const ChipAxis* axes = p.axes + (long)n * (sw + sh);

  int acc[CH_BAND][CH_PER];
#pragma unroll
  for (int k = 0; k < CH_BAND; ++k)
#pragma unroll
    for (int i = 0; i < CH_PER; ++i) acc[k][i] = 1 << (LB_PRECISION_BITS - 1);

  // the resized rows of this band, [y_first, y_last), and the source rows all their windows cover
  const int y_first = max(Y0 - dy, 0), y_last = min(Y0 + rows_here - dy, nh);
  int lo = 0, hi = 0;
  if (y_first < y_last) {
    const ChipTaps a = chip_taps(axes[sw + y_first], y_first, h, nh), z = chip_taps(axes[sw + y_last - 1], y_last - 1, h, nh);
    lo = a.xmin;
    hi = max(z.xmin + z.n, lo);
  }
  const unsigned char* src = p.frames + 3L * ((long)rec.image * p.ihm * p.iwm + (long)q.y * p.iwm + q.x);
  const long pitch = 3L * p.iwm;
  // The horizontal weights are the same for every source row.  Where all of them fit (kh taps an index, Pillow's ksize, at
  // most CH_WCACHE in all) they are recomputed once per workgroup, tap-major so that lanes along a row read along the banks;
  // beyond that every tap is recomputed where it is used.  The same integers either way: no size changes a byte.
  const int kh = lo < hi ? lb_ksize(w, nw) : 0;
  const bool cached = (long)kh * nw <= CH_WCACHE;
  if (cached) {
    for (int i = tid; i < kh * nw; i += 256) {
      const int x = i / nw, xx = i - x * nw;
      const ChipTaps k = chip_taps(axes[xx], xx, w, nw);
      s_wh[i] = x < k.n ? chip_weight(k, x) : 0;
    }
    __syncthreads();
  }
  for (int y0 = lo; y0 < hi; y0 += CH_CHUNK) {
    const int rows = min(CH_CHUNK, hi - y0);
    // horizontal: one resized pixel of one chunk row per item, consecutive lanes along the row
    for (int item = tid; item < rows * nw; item += 256) {
      const int r = item / nw, xx = item - r * nw;
      const ChipAxis a = axes[xx];
      const int xmin = vr_clampi(a.xmin, 0, w), n = vr_clampi(a.n, 0, w - xmin);         // no tap leaves the crop
      const unsigned char* s = src + (long)(y0 + r) * pitch + 3L * xmin;
      int a0 = 1 << (LB_PRECISION_BITS - 1), a1 = a0, a2 = a0;
      if (cached) {
        const int taps = min(n, kh);                  // n <= ksize in Resample.c: the min never acts
        for (int x = 0; x < taps; ++x) {
          const int wt = s_wh[x * nw + xx];
          a0 += wt * s[3 * x];
          a1 += wt * s[3 * x + 1];
          a2 += wt * s[3 * x + 2];
        }
      } else {
        const ChipTaps k = chip_taps(a, xx, w, nw);
        for (int x = 0; x < n; ++x) {
          const int wt = chip_weight(k, x);
          a0 += wt * s[3 * x];
          a1 += wt * s[3 * x + 1];
          a2 += wt * s[3 * x + 2];
        }
      }
      unsigned char* m = s_mid + r * Dm + 3 * xx;
      m[0] = clip8(a0);
      m[1] = clip8(a1);
      m[2] = clip8(a2);
    }
    if (tid < CH_CHUNK * CH_BAND) {                 // the vertical weights of the chunk: 0 outside a row's window
      const int r = tid / CH_BAND, k = tid % CH_BAND, yy = Y0 + k - dy, y = y0 + r;
      int wt = 0;
      if (r < rows && yy >= y_first && yy < y_last) {
        const ChipTaps t = chip_taps(axes[sw + yy], yy, h, nh);
        if (y >= t.xmin && y < t.xmin + t.n) wt = chip_weight(t, y - t.xmin);
      }
      s_wv[tid] = wt;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
#pragma unroll
      for (int k = 0; k < CH_BAND; ++k) {
        const int wt = s_wv[r * CH_BAND + k];       // wave-uniform
        if (wt == 0) continue;
#pragma unroll
        for (int i = 0; i < CH_PER; ++i) {
          const int j = tid + 256 * i - 3 * dx;     // the byte of the resized row under chip byte tid + 256 i
          if (j >= 0 && j < Dm) acc[k][i] += wt * s_mid[r * Dm + j];
        }
      }
    }
    __syncthreads();                                // s_mid and s_wv are rewritten by the next chunk
  }

  // clip, paste on grey, store; the band's chip rows are one contiguous block of rows_here D bytes
  unsigned char* out = p.chips + ((long)n * sh + Y0) * D;
#pragma unroll
  for (int k = 0; k < CH_BAND; ++k) {
    const int yy = Y0 + k - dy;
#pragma unroll
    for (int i = 0; i < CH_PER; ++i) {
      const int c = tid + 256 * i, j = c - 3 * dx;
      if (k < rows_here && c < D) {
        const unsigned char v = (yy >= 0 && yy < nh && j >= 0 && j < Dm) ? clip8(acc[k][i]) : (unsigned char)128;
        out[k * D + c] = v;
        s_mid[k * D + c] = v;
      }
    }
  }
  if (p.chips_f32) {                                // uniform: one thread per chip pixel of the band
    __syncthreads();
    const long HW = (long)sh * sw;
    for (int r = tid; r < rows_here * sw; r += 256) normalise_store(p.chips_f32, n, HW, (long)Y0 * sw + r, s_mid + 3 * r);
  }
}

}  // namespace

extern "C" long vrnet_chip_workspace(int n_cap, int sh, int sw) {
  if (n_cap < 1 || n_cap > (1 << 20) || sh < 1 || sh > CH_MAX || sw < 1 || sw > CH_MAX) return -1;
  return (long)n_cap * (sh + sw) * (long)sizeof(ChipAxis);
}

extern "C" int vrnet_chip_boxes_u8(const unsigned char* frames, int B, int ihm, int iwm, const vrnet_frame_geom* geom,
                                   const int* rows, const int* offsets, int n_cap, int sh, int sw, int letterbox,
                                   unsigned char* chips, float* chips_f32, vrnet_chip_rec* table, int* summary, void* workspace,
                                   int* flag, void* stream) {
  static_assert(sizeof(ChipAxis) == 16 && sizeof(vrnet_chip_rec) == 32, "chip_boxes: record layouts");
  VR_CHECK_ARG(frames && rows && offsets && chips && table && summary && workspace,
               "chip_boxes: frames, rows, offsets, chips, table, summary and workspace are required");
  VR_CHECK_ARG(B > 0 && B < 65536 && ihm > 0 && iwm > 0 && (long)ihm * iwm < (1L << 31),
               "chip_boxes: bad shape (B %d, slots of %d x %d; 1..65535 images, below 2^31 pixels each)", B, ihm, iwm);
  VR_CHECK_ARG(n_cap > 0 && n_cap <= (1 << 20) && sh >= 1 && sh <= CH_MAX && sw >= 1 && sw <= CH_MAX,
               "chip_boxes: %d rows outside [1, 2^20] or chips of %d x %d outside [1, %d]", n_cap, sh, sw, CH_MAX);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(chips_f32) & 3) == 0,
               "chip_boxes: the workspace must be 8-byte aligned, the table and the float chips 4-byte aligned");
  const ChipArgs p{frames, geom, rows, offsets, chips, chips_f32, table, summary, static_cast<ChipAxis*>(workspace), flag,
                   B, ihm, iwm, n_cap, sh, sw, letterbox != 0};
  hipLaunchKernelGGL(chip_tables_kernel, dim3((unsigned int)n_cap), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("chip_boxes (tables)");
  const int bands = (sh + CH_BAND - 1) / CH_BAND;
  hipLaunchKernelGGL(chip_resample_kernel, dim3((unsigned int)n_cap * bands), dim3(256), 0, vr_stream(stream), p, bands);
  VR_LAUNCH_CHECK("chip_boxes (resample)");
  return VR_OK;
}
