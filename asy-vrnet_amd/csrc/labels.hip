// The label of every detection on the rendered frame, yolo.py:210-224: the filled tag in the class colour and
// "<class name> <score:.2f>" in black on it, over the picture vrnet_render_u8 finished.  A label is a class name and one of
// the 101 strings 0.00 .. 1.00, so the host rasterises all num_classes x 101 of them once with Pillow itself (render.LabelAtlas:
// the "L" mask ImageDraw.text would paste, its offset, and label_size) and the device only looks masks up and blends them.
//
// THE RULE.  The rows of an image are drawn in order i = 0 .. n-1; row i paints
//   (a) its `thickness` rings, as render.hip defines them;
//   (b) the filled rectangle [ox, oy] .. [ox + size_w, oy + size_h], inclusive, clipped to the image, in the row's colour,
//       (ox, oy) = (left, top - size_h) if top - size_h >= 0, else (left, top + 1)                     (yolo.py:216-223);
//   (c) its mask at (ox + mask_off_x, oy + mask_off_y) with black ink, clipped to the image: per byte
//       v = DIV255(v * (255 - m)), DIV255(a) = ((a + 128) + ((a + 128) >> 8)) >> 8 -- Pillow's fill_mask_L / BLEND8 with ink 0.
// So the final value of a pixel: let i* be the highest row whose ring or fill covers it.  The base is the colour of i* if i*
// covers it with its fill, the byte that is there (vrnet_render_u8 painted the ring) if i* is a ring or there is no i*; then
// the masks of the rows j >= i* (all rows without an i*) that cover the pixel with m > 0 are applied in ascending j.
//
// THE KERNEL.  Work follows the label area, not the frame: the grid is (pixel blocks, row, image) and a workgroup walks the
// rectangle of its row -- the bounding box of fill and mask, clipped to the image.  Exactly one thread owns a pixel: the one
// of the HIGHEST row whose rectangle covers it; every other thread that meets the pixel leaves it alone.  The owner computes
// the whole final value by the rule above from the image's rows, staged in LDS as render_kernel stages them (1024 rows:
// 52 KiB), reads the pixel at most once and writes it at most once.  A workgroup first marks, one bit per row, the rows
// that can touch its rectangle at all, and the per-pixel scans visit those only.  No racing stores, no floating point, no atomics on
// pixels: the same bytes on every run.  Rows past RN_MAXBOX of an image are ignored (bit 4 of *flag), as render.hip ignores
// them.  Nothing from the tables is trusted: label indices are clamped, a record whose mask leaves the blob draws no text.
#include "common.h"

namespace {

constexpr int RN_MAXCOL = 256;       // as in render.hip
constexpr int RN_MAXBOX = 1024;
constexpr int RN_COORD = 1 << 29;
constexpr int RN_FLAG_BOX_ROWS = 4;
constexpr int NMS_FLAG_DET_CLASS = 16;        // nms.hip
constexpr int LB_FLAG_SCORE = 2048;           // a score that is NaN or outside [0, 1], clamped
constexpr int LB_SCORES = 101;                // 0.00 .. 1.00
constexpr int LB_REC = 8;                     // int32 per record: blob offset, mask w, h, mask offset x, y, label_size w, h, 0
constexpr int LB_MAXDIM = 1 << 14;            // a mask or label side, and a mask offset, are clamped to this
constexpr int LB_XBLOCKS = 4;                 // workgroups per row; each strides over the row's rectangle

struct LabelArgs {
  unsigned char* pic;                // (B, ih, iw, 3), in place
  const int* boxes;                  // (n_rows, 5)
  const int* offsets;                // (B + 1)
  const int* label_idx;              // (n_rows): class * 101 + k
  const unsigned char* box_palette;  // (n_box_colors, 3)
  const unsigned char* blob;         // (blob_bytes)
  const int* recs;                   // (n_sizes, n_labels, LB_REC)
  const int* size_tab;               // RAGGED: (B) size index of image b, -1 = no labels
  const vrnet_frame_geom* tab;       // RAGGED: (B)
  int* flag;
  long blob_bytes;
  int B, ih, iw, n_rows, n_box_colors, n_labels, n_sizes, size_index, thickness;
};

__device__ __forceinline__ unsigned int div255(unsigned int a) {
  a += 128u;
  return (a + (a >> 8)) >> 8;
}

__device__ __forceinline__ bool on_rings(int x, int y, const int4 q, int thickness) {
  const int dx = min(x - q.x, q.z - x), dy = min(y - q.y, q.w - y);
  return (unsigned int)min(dx, dy) < (unsigned int)thickness;
}

// fill: x0, y0, x1, y1 inclusive; text: x, y, w, h
__device__ __forceinline__ bool in_fill(int x, int y, const int4 f) { return x >= f.x && x <= f.z && y >= f.y && y <= f.w; }
__device__ __forceinline__ bool in_text(int x, int y, const int4 t) {
  return (unsigned int)(x - t.x) < (unsigned int)t.z && (unsigned int)(y - t.y) < (unsigned int)t.w;
}
// the row's rectangle: the bounding box of fill and mask, inclusive
__device__ __forceinline__ int4 row_rect(const int4 f, const int4 t) {
  if (t.z <= 0 || t.w <= 0) return f;
  return make_int4(min(f.x, t.x), min(f.y, t.y), max(f.z, t.x + t.z - 1), max(f.w, t.y + t.w - 1));
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void labels_kernel(const LabelArgs p) {
  __shared__ int4 s_box[RN_MAXBOX], s_fill[RN_MAXBOX], s_text[RN_MAXBOX];
  __shared__ int s_off[RN_MAXBOX];
  __shared__ unsigned char s_col[RN_MAXBOX];
  __shared__ unsigned long long s_rel[RN_MAXBOX / 64];
  const int tid = threadIdx.x, r = blockIdx.y, b = blockIdx.z;
  const bool first = blockIdx.x == 0 && r == 0 && tid == 0;
  int ih = p.ih, iw = p.iw, thickness = p.thickness, sidx = p.size_index;
  if constexpr (RAGGED) {                             // the image's own record: the block's, so wave-uniform
    bool bad;
    const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ih, p.iw, 0, 0, bad);
    sidx = p.size_tab[b];
    if (first && (bad || sidx >= p.n_sizes) && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
    ih = g.ih; iw = g.iw; thickness = g.thickness;
    if (sidx < 0 || sidx >= p.n_sizes) return;        // no labels for this image
  }
  int start, n;
  vr_row_range(p.offsets, b, p.n_rows, start, n);
  if (n > RN_MAXBOX) {
    if (first && p.flag) atomicOr(p.flag, RN_FLAG_BOX_ROWS);
    n = RN_MAXBOX;
  }
  if (r >= n) return;                                 // the whole workgroup
  const int* recs = p.recs + (long)sidx * p.n_labels * LB_REC;
  for (int k = tid; k < n; k += 256) {
    const int* row = p.boxes + 5L * (start + k);
    const int left = vr_clampi(row[0], -RN_COORD, RN_COORD), top = vr_clampi(row[1], -RN_COORD, RN_COORD);
    s_box[k] = make_int4(left, top, vr_clampi(row[2], -RN_COORD, RN_COORD), vr_clampi(row[3], -RN_COORD, RN_COORD));
    s_col[k] = (unsigned char)vr_clampi(row[4], 0, p.n_box_colors - 1);
    const int* rec = recs + (long)vr_clampi(p.label_idx[start + k], 0, p.n_labels - 1) * LB_REC;
    const int off = rec[0];
    int mw = vr_clampi(rec[1], 0, LB_MAXDIM), mh = vr_clampi(rec[2], 0, LB_MAXDIM);
    const int mox = vr_clampi(rec[3], -LB_MAXDIM, LB_MAXDIM), moy = vr_clampi(rec[4], -LB_MAXDIM, LB_MAXDIM);
    const int lw = vr_clampi(rec[5], 0, LB_MAXDIM), lh = vr_clampi(rec[6], 0, LB_MAXDIM);
    if (off < 0 || (long)off + (long)mw * mh > p.blob_bytes) mw = mh = 0;      // a mask outside the blob: no text
    const int ox = left, oy = top - lh >= 0 ? top - lh : top + 1;
    s_fill[k] = make_int4(ox, oy, ox + lw, oy + lh);
    s_text[k] = make_int4(ox + mox, oy + moy, mw, mh);
    s_off[k] = off;
  }
  __syncthreads();
  int4 R = row_rect(s_fill[r], s_text[r]);
  R.x = max(R.x, 0); R.y = max(R.y, 0); R.z = min(R.z, iw - 1); R.w = min(R.w, ih - 1);
  if (R.x > R.z || R.y > R.w) return;                 // the whole workgroup: R is the row's
  // the rows that can touch a pixel of R at all: their rectangle meets R (ownership, fill, text), or their rings do -- the
  // box meets R and R does not lie inside the hollow the rings leave.  One bit per row, so the scans below keep the order.
  for (int w = tid; w < RN_MAXBOX / 64; w += 256) s_rel[w] = 0ull;
  __syncthreads();
  for (int k = tid; k < n; k += 256) {
    const int4 q = row_rect(s_fill[k], s_text[k]), bx = s_box[k];
    const bool meets = q.x <= R.z && q.z >= R.x && q.y <= R.w && q.w >= R.y;
    const bool rings = bx.x <= R.z && bx.z >= R.x && bx.y <= R.w && bx.w >= R.y &&
                       !(R.x >= bx.x + thickness && R.z <= bx.z - thickness && R.y >= bx.y + thickness && R.w <= bx.w - thickness);
    if (meets || rings) atomicOr(&s_rel[k >> 6], 1ull << (k & 63));
  }
  __syncthreads();
  const int RW = R.z - R.x + 1;
  const long npix = (long)RW * (R.w - R.y + 1);
  unsigned char* img = p.pic + 3L * b * p.ih * p.iw;  // the slot; rows of p.iw pixels
  for (long t = (long)blockIdx.x * 256 + tid; t < npix; t += (long)gridDim.x * 256) {
    const int y = R.y + (int)(t / RW), x = R.x + (int)(t % RW);
    // one pass from the last row down.  Above r: a rectangle that covers the pixel owns it (this thread leaves), a ring
    // that covers it is i*.  From r down: the first ring or fill is i*, unless a ring above r already was.
    int istar = -1;
    bool filled = false, owned = true, done = false;
    for (int w = (n - 1) >> 6; w >= 0 && owned && !done; --w) {
      unsigned long long bits = s_rel[w];
      while (bits) {
        const int j = (w << 6) + 63 - __clzll((long long)bits);
        bits &= ~(1ull << (j & 63));
        if (j > r) {
          const int4 q = row_rect(s_fill[j], s_text[j]);
          if (x >= q.x && x <= q.z && y >= q.y && y <= q.w) { owned = false; break; }
          if (istar < 0 && on_rings(x, y, s_box[j], thickness)) istar = j;
        } else {
          if (istar >= 0) { done = true; break; }
          filled = in_fill(x, y, s_fill[j]);
          if (filled || on_rings(x, y, s_box[j], thickness)) { istar = j; done = true; break; }
        }
      }
    }
    if (!owned) continue;
    unsigned char* o = img + 3L * ((long)y * p.iw + x);
    unsigned int v0, v1, v2;
    if (filled) {
      const unsigned char* c = p.box_palette + 3 * s_col[istar];
      v0 = c[0]; v1 = c[1]; v2 = c[2];
    } else {
      v0 = o[0]; v1 = o[1]; v2 = o[2];
    }
    // the masks of the rows j >= i* in ascending order; a mask lies inside its row's rectangle, and no rectangle above r
    // covers an owned pixel, so the rows max(i*, 0) .. r are all there is
    bool inked = false;
    const int lo = max(istar, 0);
    for (int w = lo >> 6; w <= (r >> 6) && lo <= r; ++w) {
      unsigned long long bits = s_rel[w];
      if (w == (lo >> 6)) bits &= ~0ull << (lo & 63);
      if (w == (r >> 6) && (r & 63) != 63) bits &= (1ull << ((r & 63) + 1)) - 1ull;
      while (bits) {
        const int j = (w << 6) + __ffsll((long long)bits) - 1;
        bits &= bits - 1ull;
        const int4 tx = s_text[j];
        if (!in_text(x, y, tx)) continue;
        const unsigned int m = p.blob[(long)s_off[j] + (long)(y - tx.y) * tx.z + (x - tx.x)];
        if (!m) continue;
        v0 = div255(v0 * (255u - m));
        v1 = div255(v1 * (255u - m));
        v2 = div255(v2 * (255u - m));
        inked = true;
      }
    }
    if (filled || inked) {
      o[0] = (unsigned char)v0;
      o[1] = (unsigned char)v1;
      o[2] = (unsigned char)v2;
    }
  }
}

// k of '{:.2f}'.format(s): the exact value m 2^-sh of the fp32 times 100, rounded to nearest with ties to even, in integers
__device__ __forceinline__ int score_index(float s, bool& bad) {
  bad = !(s >= 0.0f && s <= 1.0f);
  if (bad) return s > 1.0f ? 100 : 0;                 // NaN and negatives: 0
  const unsigned int bits = __float_as_uint(s);
  const int e = (int)((bits >> 23) & 255u);
  const unsigned long long m = (bits & 0x7FFFFFu) | (e ? 0x800000u : 0u);
  const int sh = 150 - (e ? e : 1);                   // s = m 2^-sh, sh >= 23 for s <= 1
  if (sh >= 32) return 0;                             // 100 m < 2^31 <= half an ulp of the integer grid
  const unsigned long long N = 100ull * m, q = N >> sh, rem = N & ((1ull << sh) - 1ull), half = 1ull << (sh - 1);
  return (int)(q + ((rem > half || (rem == half && (q & 1ull))) ? 1ull : 0ull));
}

struct IndexArgs {
  const float* rows;                 // (B, cap, 7): .., obj, class_conf, class
  const int* kept;                   // (B)
  const int* offsets;                // (B + 1)
  int* out;                          // (n_out)
  int* flag;
  int B, cap, nc, n_out;
};

__global__ __launch_bounds__(256) void label_index_kernel(const IndexArgs p) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k >= min(max(p.kept[b], 0), p.cap)) return;
  const long pos = (long)p.offsets[b] + k;
  if (pos < 0 || pos >= p.n_out) return;
  const float* r = p.rows + ((long)b * p.cap + k) * 7;
  bool bad;
  const int idx = score_index(r[4] * r[5], bad);      // one fp32 multiply (yolo.py:157)
  if (bad && p.flag) atomicOr(p.flag, LB_FLAG_SCORE);
  const int label = (int)r[6];
  if ((label < 0 || label >= p.nc) && p.flag) atomicOr(p.flag, NMS_FLAG_DET_CLASS);
  p.out[pos] = vr_clampi(label, 0, p.nc - 1) * LB_SCORES + idx;
}

int labels_check(const char* fn, const LabelArgs& p, int num_classes) {
  VR_CHECK_ARG(p.pic && p.B > 0 && p.B < 65536 && p.ih > 0 && p.iw > 0 && p.ih <= (1 << 24) && p.iw <= (1 << 24) &&
                   (long)p.B * p.ih * p.iw < (1L << 31),
               "%s: bad shape (B %d, %d x %d; at most 2^31 - 1 pixels in all)", fn, p.B, p.ih, p.iw);
  VR_CHECK_ARG(p.n_rows >= 0 && (p.n_rows == 0 || (p.boxes && p.offsets && p.label_idx && p.box_palette && p.n_box_colors > 0 &&
                                                    p.n_box_colors <= RN_MAXCOL)),
               "%s: %d rows need boxes, offsets, label indices and a box palette of 1..%d colours", fn, p.n_rows, RN_MAXCOL);
  VR_CHECK_ARG(p.recs && num_classes >= 1 && num_classes <= RN_MAXCOL && p.n_sizes >= 1 && p.n_sizes <= 65536 && p.blob_bytes >= 0 &&
                   p.blob_bytes < (1L << 31) && (p.blob || p.blob_bytes == 0),
               "%s: the atlas needs records, 1..%d classes, 1..65536 sizes and a blob below 2 GiB", fn, RN_MAXCOL);
  return VR_OK;
}

template <bool RAGGED>
int labels_launch(const char* fn, const LabelArgs& p, void* stream) {
  if (p.n_rows == 0) return VR_OK;
  const int rows = p.n_rows < RN_MAXBOX ? p.n_rows : RN_MAXBOX;
  // one workgroup of row 0 always exists, so more than RN_MAXBOX rows in an image are reported
  hipLaunchKernelGGL(labels_kernel<RAGGED>, dim3(LB_XBLOCKS, rows, p.B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK(fn);
  return VR_OK;
}

}  // namespace

extern "C" int vrnet_label_index_f32(const float* rows, const int* kept, const int* offsets, int B, int cap, int num_classes,
                                     int* label_idx, int n_out, int* flag, void* stream) {
  VR_CHECK_ARG(rows && kept && offsets && label_idx && B > 0 && B < 65536 && cap > 0 && (long)B * cap < (1L << 27) &&
                   num_classes >= 1 && num_classes <= RN_MAXCOL && n_out >= 0,
               "label_index: bad arguments (B %d, cap %d, %d classes, %d outputs)", B, cap, num_classes, n_out);
  if (n_out == 0) return VR_OK;
  IndexArgs p{rows, kept, offsets, label_idx, flag, B, cap, num_classes, n_out};
  hipLaunchKernelGGL(label_index_kernel, dim3(vr_cdiv(cap, 256), B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("label_index");
  return VR_OK;
}

extern "C" int vrnet_render_labels_u8(unsigned char* picture, int B, int ih, int iw, const int* boxes, const int* box_offsets,
                                      int n_rows, const unsigned char* box_palette, int n_box_colors, int thickness,
                                      const int* label_idx, const unsigned char* blob, long blob_bytes, const int* records,
                                      int num_classes, int n_sizes, int size_index, int* flag, void* stream) {
  LabelArgs p{};
  p.pic = picture; p.boxes = boxes; p.offsets = box_offsets; p.label_idx = label_idx; p.box_palette = box_palette;
  p.blob = blob; p.recs = records; p.flag = flag; p.blob_bytes = blob_bytes;
  p.B = B; p.ih = ih; p.iw = iw; p.n_rows = n_rows; p.n_box_colors = n_box_colors; p.n_labels = num_classes * LB_SCORES;
  p.n_sizes = n_sizes; p.size_index = size_index; p.thickness = thickness;
  if (const int rc = labels_check("render_labels", p, num_classes)) return rc;
  VR_CHECK_ARG(size_index >= 0 && size_index < n_sizes && thickness > 0 && thickness <= (1 << 24),
               "render_labels: size index %d outside [0, %d) or thickness %d outside [1, 2^24]", size_index, n_sizes, thickness);
  return labels_launch<false>("render_labels", p, stream);
}

extern "C" int vrnet_render_labels_ragged_u8(unsigned char* picture, const vrnet_frame_geom* geom, const int* size_index, int B,
                                             int ihm, int iwm, const int* boxes, const int* box_offsets, int n_rows,
                                             const unsigned char* box_palette, int n_box_colors, const int* label_idx,
                                             const unsigned char* blob, long blob_bytes, const int* records, int num_classes,
                                             int n_sizes, int* flag, void* stream) {
  LabelArgs p{};
  p.pic = picture; p.boxes = boxes; p.offsets = box_offsets; p.label_idx = label_idx; p.box_palette = box_palette;
  p.blob = blob; p.recs = records; p.flag = flag; p.blob_bytes = blob_bytes; p.tab = geom; p.size_tab = size_index;
  p.B = B; p.ih = ihm; p.iw = iwm; p.n_rows = n_rows; p.n_box_colors = n_box_colors; p.n_labels = num_classes * LB_SCORES;
  p.n_sizes = n_sizes;
  if (const int rc = labels_check("render_labels_ragged", p, num_classes)) return rc;
  VR_CHECK_ARG(geom && size_index, "render_labels_ragged: needs the geometry table and the size-index table");
  return labels_launch<true>("render_labels_ragged", p, stream);
}
