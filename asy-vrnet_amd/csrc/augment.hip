// The random training augmentation of the reference's dataloaders, on the device and from raw bytes: the recipe of
// utils/dataloader.py:187-247 (random resize with aspect jitter, random placement on the grey canvas, left-right flip, HSV
// jitter, the boxes mapped alongside), extended to the label map as utils_seg/dataloader.py:91-111 treats it and to the radar
// map by this project's own definition (data.augment_sample).  Nothing here is random: the host draws one vrnet_aug_rec per
// image (data.augment_params) and these kernels apply it, so they equal the host functions of data.py bit for bit.
// Differences to the letterbox of csrc/letterbox.hip, whose arithmetic (resample.h) they share:
//   the window (nw x nh at (dx, dy)) may be larger than the canvas and start at negative offsets: Pillow's paste crops it.
//     Tables, the horizontal result and every index below are by VISIBLE window column / row -- window column x0 + v is
//     visible column v, x0 = max(0, -dx), at most W of them -- so the workspace is vrnet_letterbox_ragged_workspace's; the
//     taps themselves are those of the full iw -> nw axis (bicubic_taps_at), the nearest recurrence runs from column 0
//   the flip is an index: canvas column x reads what column W - 1 - x of the unflipped canvas holds
//   the colour stage (data.hsv_jitter): RGB -> HSV in OpenCV's 8-bit integer arithmetic, three 256-byte tables from the
//     record, HSV -> RGB in float32 with one rounding per operation.  The 768 table bytes and the two divisor tables of
//     the forward conversion are staged in LDS per workgroup
// Kernels (grid y = image, the record loaded wave-uniformly and clamped by aug_load so that no access leaves the slot, the
// canvas or the workspace; VR_FLAG_GEOMETRY reports a clamped record or taps beyond the capacity):
//   tables      bounds and taps of the visible columns and rows, one thread each
//   horizontal  (ih, iw, 3) -> (ih, visible columns, 3) in the workspace; an image with nw == iw skips it, as Pillow does
//   vertical    one thread per canvas pixel: vertical taps (a copy when nh == ih), paste, flip, colour, normalise_store;
//               consecutive lanes store consecutive x
//   seg         seg_targets_ragged_kernel's body with the visible-index tables and the flip
//   boxes       box_targets_ragged_kernel's arithmetic with the record's window and the flip before the clip
//   radar       an integer gather of the stored map, (B, 4, H, W) -> (B, 4, H, W)
// The tap sum is resample.h's; the paste epilogue, the one-hot store, the box rules and the radar pick are augment.h's.
#include "augment.h"

#pragma clang fp contract(off)

extern "C" {
/* include/vrnet_hip.h: the per-image augmentation record (816 bytes). */
typedef struct vrnet_aug_rec {
  int ih, iw;                        /* the image's own size inside its (ihm, iwm) slot */
  int nw, nh, dx, dy;                /* the resized frame and where it is pasted; may leave the canvas on every side */
  int flip, color;                   /* != 0: mirror the canvas left-right; run the colour stage */
  int lb_nw, lb_nh, lb_dx, lb_dy;    /* data.letterbox_geometry: the window the stored radar map is aligned with */
  unsigned char lut[3][256];         /* hue, saturation, value tables of the colour stage */
} vrnet_aug_rec;
}
static_assert(sizeof(vrnet_aug_rec) == 816 && alignof(vrnet_aug_rec) == 4, "vrnet_aug_rec layout");

namespace {

constexpr int AUG_HEAD_INTS = 12;

struct AugRec {
  int ih, iw, nw, nh, dx, dy, flip, color, lb_nw, lb_nh, lb_dx, lb_dy;
  int x0, y0, nvx, nvy;              // first visible window column / row and how many are visible (<= W, <= H)
  bool empty;                        // no pixels, or a bad record: every output of the image is padding
};

// Record b, clamped: 0 <= ih <= ihm, 0 <= iw <= iwm; 0 <= nw, nh <= 2 max(W, H) (what scale <= 2 can give); -nw <= dx <= W and
// -nh <= dy <= H (beyond: nothing visible either way); the letterbox window inside the canvas.  bad: something was clamped,
// or a size or window is not positive; the image is then `empty`.  b is the block's image, so the twelve loads are wave-uniform.
__device__ __forceinline__ AugRec aug_load(const vrnet_aug_rec* tab, int b, int ihm, int iwm, int H, int W, bool& bad) {
  const int* t = reinterpret_cast<const int*>(tab + b);
  AugRec g;
  const int lim = 2 * (W > H ? W : H);
  g.ih = vr_clampi(t[0], 0, ihm);
  g.iw = vr_clampi(t[1], 0, iwm);
  g.nw = vr_clampi(t[2], 0, lim);
  g.nh = vr_clampi(t[3], 0, lim);
  g.dx = vr_clampi(t[4], -g.nw, W);
  g.dy = vr_clampi(t[5], -g.nh, H);
  g.flip = t[6] != 0;
  g.color = t[7] != 0;
  g.lb_nw = vr_clampi(t[8], 0, W);
  g.lb_nh = vr_clampi(t[9], 0, H);
  g.lb_dx = vr_clampi(t[10], 0, W - g.lb_nw);
  g.lb_dy = vr_clampi(t[11], 0, H - g.lb_nh);
  bad = g.ih != t[0] || g.iw != t[1] || g.nw != t[2] || g.nh != t[3] || g.dx != t[4] || g.dy != t[5] || g.lb_nw != t[8] ||
        g.lb_nh != t[9] || g.lb_dx != t[10] || g.lb_dy != t[11] || t[0] <= 0 || t[1] <= 0 || t[2] <= 0 || t[3] <= 0 ||
        t[8] <= 0 || t[9] <= 0;
  // a record that had to be clamped is not applied in part: its image is all padding (and reported), whatever the host
  // meant by it; the clamped values above only keep every index derived from them in range
  g.empty = bad || g.ih <= 0 || g.iw <= 0 || g.nw <= 0 || g.nh <= 0;
  if (bad) g.color = 0;
  g.x0 = g.dx < 0 ? -g.dx : 0;
  g.y0 = g.dy < 0 ? -g.dy : 0;
  const int xe = g.nw < W - g.dx ? g.nw : W - g.dx, ye = g.nh < H - g.dy ? g.nh : H - g.dy;
  g.nvx = g.empty || xe < g.x0 ? 0 : xe - g.x0;          // xe - x0 <= W - dx - x0 <= W
  g.nvy = g.empty || ye < g.y0 ? 0 : ye - g.y0;
  return g;
}

struct AugFramesArgs {
  const unsigned char* img;          // (B, ihm, iwm, 3)
  const vrnet_aug_rec* tab;          // (B)
  int B, ihm, iwm, H, W, cap;        // cap: taps per table entry
  long slot;                         // ints of one image's tables
  int* tables;
  unsigned char* mid;                // (B, ihm, W, 3): the horizontal pass's result, rows of W visible columns
  unsigned char* canvas;             // (B, H, W, 3) or null
  float* images;                     // (B, 3, H, W) or null
  int* flag;                         // or null
};

struct AugTables {
  int *hb, *hk, *vb, *vk;            // taps of visible column v: hk[t * W + v]; of visible row v: vk[t * H + v]
};

__device__ __forceinline__ AugTables aug_tables(const AugFramesArgs& p, int b) {
  AugTables s;
  int* t = p.tables + b * p.slot;
  s.hb = t; t += 2L * p.W;
  s.hk = t; t += (long)p.W * p.cap;
  s.vb = t; t += 2L * p.H;
  s.vk = t;
  return s;
}

__global__ __launch_bounds__(256) void augment_tables_kernel(const AugFramesArgs p) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const AugRec g = aug_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  if (e == 0 && p.flag) {            // a clamped record, or taps beyond the slot's capacity (bicubic_taps_at then truncates them)
    if (!g.empty) bad = bad || (g.nw != g.iw && lb_ksize(g.iw, g.nw) > p.cap) || (g.nh != g.ih && lb_ksize(g.ih, g.nh) > p.cap);
    if (bad) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  }
  if (g.empty) return;
  const AugTables s = aug_tables(p, b);
  if (e < p.W) {
    if (e < g.nvx && g.nw != g.iw) bicubic_taps_at(g.x0 + e, g.iw, g.nw, p.cap, s.hb, s.hk, e, p.W);
  } else if (e < p.W + p.H) {
    const int v = e - p.W;
    if (v < g.nvy && g.nh != g.ih) bicubic_taps_at(g.y0 + v, g.ih, g.nh, p.cap, s.vb, s.vk, v, p.H);
  }
}

__global__ __launch_bounds__(256) void augment_horizontal_kernel(const AugFramesArgs p) {
  const int b = blockIdx.y;
  bool bad;
  const AugRec g = aug_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  if (g.empty || g.nw == g.iw) return;             // this image skips the pass, as Pillow does
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(e / p.W), v = (int)(e - (long)row * p.W);
  if (row >= g.ih || v >= g.nvx) return;
  const AugTables s = aug_tables(p, b);
  const int xmin = s.hb[2 * v], n = s.hb[2 * v + 1];            // xmin + n <= iw: inside the slot's row
  const unsigned char* src = p.img + (((long)b * p.ihm + row) * p.iwm + xmin) * 3;
  resample_taps3(src, 3, s.hk + v, p.W, n, p.mid + (((long)b * p.ihm + row) * p.W + v) * 3);
}

__global__ __launch_bounds__(256) void augment_vertical_paste_kernel(const AugFramesArgs p) {
  __shared__ ColorLds c;
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const AugRec g = aug_load(p.tab, (int)b, p.ihm, p.iwm, p.H, p.W, bad);
  if (g.color) {                     // block-uniform
    // the 768 table bytes sit at byte 48 of the 816-byte record: 4-byte aligned words
    color_lds_fill(c, reinterpret_cast<const unsigned*>(reinterpret_cast<const int*>(p.tab + b) + AUG_HEAD_INTS));
  }
  if (r >= HW) return;
  const AugTables s = aug_tables(p, (int)b);
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const int wx = (g.flip ? p.W - 1 - x : x) - g.dx, wy = y - g.dy;
  const bool inside = !g.empty && wx >= 0 && wx < g.nw && wy >= 0 && wy < g.nh;
  unsigned char v[3] = {128, 128, 128};
  if (inside) {
    // the horizontal result: the workspace (rows of W visible columns), or the frame's own slot when that pass was skipped
    const bool resized = g.nw != g.iw;
    const unsigned char* src = resized ? p.mid + (b * p.ihm * p.W + (wx - g.x0)) * 3 : p.img + (b * p.ihm * p.iwm + wx) * 3;
    const long rs = (resized ? (long)p.W : (long)p.iwm) * 3;
    if (g.nh != g.ih) {
      const int vy = wy - g.y0;
      const int ymin = s.vb[2 * vy], n = s.vb[2 * vy + 1];
      resample_taps3(src + ymin * rs, rs, s.vk + vy, p.H, n, v);
    } else {
      src += wy * rs;
      v[0] = src[0];
      v[1] = src[1];
      v[2] = src[2];
    }
  }
  paste_store(c, g.color, v, p.canvas, p.images, b, HW, r);
}

// ---- the segmentation targets: seg_targets_ragged_kernel (csrc/traintargets.hip) under the record's window and flip ------
struct AugSegArgs {
  const unsigned char* label;        // (B, ihm, iwm)
  const vrnet_aug_rec* tab;          // (B)
  int B, ihm, iwm, H, W, ns;
  int vec4;                          // W * (ns + 1) % 4 == 0 and onehot 16-byte aligned: every chunk is whole float4s
  long long* png_out;                // (B, H, W)
  float* onehot;                     // (B, H, W, ns + 1)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void augment_seg_targets_kernel(const AugSegArgs p) {
  extern __shared__ int st_lds[];
  int* xi = st_lds;                  // (W) source column of VISIBLE window column
  int* yi = xi + p.W;                // (H) source row of visible window row
  unsigned char* cls = reinterpret_cast<unsigned char*>(yi + p.H);          // (ST_ROWS * W) the clamped label of a pixel
  const int b = blockIdx.y, y0 = blockIdx.x * ST_ROWS;
  const int rows = p.H - y0 < ST_ROWS ? p.H - y0 : ST_ROWS;
  const int npix = rows * p.W, n1 = p.ns + 1;
  bool bad;
  const AugRec g = aug_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  // block-uniform: rows that miss the window are all padding and need no tables
  const bool hit = g.nvx > 0 && g.nvy > 0 && y0 < g.dy + g.nh && y0 + rows > g.dy;
  if (hit) {
    if (threadIdx.x == 0) vr_nearest_indices_from(g.iw, g.nw, g.x0, g.nvx, xi);
    if (threadIdx.x == 64) vr_nearest_indices_from(g.ih, g.nh, g.y0, g.nvy, yi);      // another wave: side by side
  }
  __syncthreads();
  const unsigned char* src = p.label + (long)b * p.ihm * p.iwm;
  long long* png = p.png_out + ((long)b * p.H + y0) * p.W;
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int r = i / p.W, x = i - r * p.W;
    const int wx = (g.flip ? p.W - 1 - x : x) - g.dx, wy = y0 + r - g.dy;
    int lab = 0;
    if (hit && wx >= 0 && wx < g.nw && wy >= 0 && wy < g.nh) {              // visible: x0 <= wx < x0 + nvx, the same for wy
      const int sx = xi[wx - g.x0], sy = yi[wy - g.y0];
      if (sx >= 0 && sx < g.iw && sy >= 0 && sy < g.ih) lab = src[(long)sy * p.iwm + sx];   // ImagingScaleAffine leaves the rest unset
    }
    if (lab >= p.ns) lab = p.ns;
    cls[i] = (unsigned char)lab;
    png[i] = lab;
  }
  __syncthreads();
  float* oh = p.onehot + ((long)b * p.H + y0) * p.W * n1;
  st_store_onehot(cls, oh, npix, n1, p.vec4);
}

// ---- the box targets: box_targets_ragged_kernel under the record's window, with the flip before the clip --------------------
struct AugBoxArgs {
  const int* boxes;                  // (B, max_gt, 5)
  const int* counts;                 // (B)
  const vrnet_aug_rec* tab;          // (B)
  int B, max_gt, ihm, iwm, H, W;
  float* targets;                    // (B, max_gt, 5)
  int* counts_out;                   // (B)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void augment_box_targets_kernel(const AugBoxArgs p) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y;
  bool bad;
  const AugRec g = aug_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  const int given = p.counts[b];
  const int n = g.empty ? 0 : vr_clampi(given, 0, p.max_gt);
  if (threadIdx.x == 0 && p.flag) {
    const int bits = (bad ? VR_FLAG_GEOMETRY : 0) | (given < 0 || given > p.max_gt ? VR_FLAG_BOX_COUNT : 0);
    if (bits) atomicOr(p.flag, bits);
  }
  const int* rows = p.boxes + (long)b * p.max_gt * 5;
  float* out = p.targets + (long)b * p.max_gt * 5;
  int base = 0;                      // rows kept so far: the same in every thread
  for (int start = 0; start < n; start += 256) {
    const int i = start + threadIdx.x;
    bool keep = false;
    long long x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    int c = 0;
    if (i < n) {
      const int* r = rows + (long)i * 5;
      x1 = map_coord(r[0], g.nw, g.iw, g.dx);
      y1 = map_coord(r[1], g.nh, g.ih, g.dy);
      x2 = map_coord(r[2], g.nw, g.iw, g.dx);
      y2 = map_coord(r[3], g.nh, g.ih, g.dy);
      c = r[4];
      if (g.flip) {                  // box[:, [0, 2]] = w - box[:, [2, 0]] (dataloader.py:241), on the integer array
        const long long t = p.W - x2;
        x2 = p.W - x1;
        x1 = t;
      }
      // box_clip_keep (augment.h), written out: the call gave this kernel another instruction schedule
      if (x1 < 0) x1 = 0;
      if (y1 < 0) y1 = 0;
      if (x2 > p.W) x2 = p.W;
      if (y2 > p.H) y2 = p.H;
      keep = x2 - x1 > 1 && y2 - y1 > 1;
    }
    const int at = box_compact_slot(keep, base, s_wave);
    if (keep) box_store_cxcywh(out + (long)at * 5, x1, y1, x2, y2, c);      // at <= i < max_gt: compaction never moves a row up
    __syncthreads();                 // s_wave is rewritten by the next chunk
  }
  box_zero_tail(base, p.max_gt, out);
  if (threadIdx.x == 0) p.counts_out[b] = base;
}

// ---- the radar map: the nearest stored pixel under the pixel-centre map, integers only ------------------------------------
struct AugRadarArgs {
  const float* radar;                // (B, 4, H, W): aligned with the letterbox window of the record
  const vrnet_aug_rec* tab;          // (B)
  int B, ihm, iwm, H, W;             // ihm, iwm: only to judge the record as the other three kernels do
  float* out;                        // (B, 4, H, W)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void augment_radar_kernel(const AugRadarArgs p) {
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const AugRec g = aug_load(p.tab, (int)b, p.ihm, p.iwm, p.H, p.W, bad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  if (r >= HW) return;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const int wx = (g.flip ? p.W - 1 - x : x) - g.dx, wy = y - g.dy;
  const bool inside = !g.empty && g.lb_nw > 0 && g.lb_nh > 0 && wx >= 0 && wx < g.nw && wy >= 0 && wy < g.nh;
  const long at = inside ? radar_pick(0, wx, wy, g.nw, g.nh, g.lb_nw, g.lb_nh, g.lb_dx, g.lb_dy, p.W) : 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const long plane = (b * 4 + c) * HW;
    p.out[plane + r] = inside ? p.radar[plane + at] : 0.f;
  }
}

}  // namespace

extern "C" int vrnet_augment_frames_u8(const unsigned char* img, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H, int W,
                                       int max_taps, unsigned char* canvas, float* images, int* flag, void* workspace,
                                       long workspace_bytes, void* stream) {
  VR_CHECK_ARG(img && aug && B > 0 && B < 65536 && ihm > 0 && iwm > 0 && H > 0 && W > 0 && max_taps >= 5 && max_taps <= 4096,
               "augment_frames: bad shape (B %d, slots %d x %d, canvas %d x %d, max_taps %d)", B, ihm, iwm, H, W, max_taps);
  VR_CHECK_ARG(canvas || images, "augment_frames: no output requested");
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(aug) & 7) == 0, "augment_frames: the record table must be 8-byte aligned");
  VR_CHECK_ARG((long)B * ihm * iwm < (1L << 31) && (long)B * H * W < (1L << 31) && (long)B * ihm * W < (1L << 31) &&
                   (long)B * lb_ragged_slot_ints(H, W, max_taps) < (1L << 31) && H < (1 << 24) && W < (1 << 24),
               "augment_frames: batch too large");
  AugFramesArgs p{};
  // one table set and one horizontal result per image: vrnet_letterbox_ragged_workspace's bytes
  if (!fm_split_workspace("augment_frames", workspace, workspace_bytes, B, ihm, H, W, max_taps, p.tables, p.mid)) return VR_ERR_WORKSPACE;
  p.img = img; p.tab = aug;
  p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.cap = max_taps;
  p.slot = lb_ragged_slot_ints(H, W, max_taps);
  p.canvas = canvas; p.images = images; p.flag = flag;
  hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(augment_tables_kernel, dim3((unsigned)vr_cdiv((long)W + H, 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(augment_horizontal_kernel, dim3((unsigned)vr_cdiv((long)ihm * W, 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(augment_vertical_paste_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("augment_frames");
  return VR_OK;
}

extern "C" int vrnet_augment_seg_targets_u8(const unsigned char* label, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H,
                                            int W, int num_classes_seg, long long* png_out, float* onehot, int* flag,
                                            void* stream) {
  VR_CHECK_ARG(label && aug && png_out && onehot, "augment_seg_targets: label, aug, png_out and onehot are required");
  VR_CHECK_ARG(fm_shape_ok(B, ihm, iwm, H, W), "augment_seg_targets: bad shape (B %d, slots %d x %d, canvas %d x %d)", B, ihm, iwm, H, W);
  VR_CHECK_ARG(num_classes_seg > 0 && num_classes_seg < 255, "augment_seg_targets: 0 < num_classes_seg < 255, got %d",
               num_classes_seg);
  VR_CHECK_ARG(st_lds_bytes(H, W) <= ST_LDS_MAX, "augment_seg_targets: a %d x %d canvas needs %ld bytes of LDS, above %ld", H, W,
               st_lds_bytes(H, W), ST_LDS_MAX);
  VR_CHECK_ARG((long)B * ihm * iwm < (1L << 31) && (long)B * H * W * (num_classes_seg + 1) < (1L << 40) &&
                   (long)ST_ROWS * W * (num_classes_seg + 1) < (1L << 31),
               "augment_seg_targets: batch too large");
  AugSegArgs p{};
  p.label = label; p.tab = aug;
  p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.ns = num_classes_seg;
  p.vec4 = ((long)W * (num_classes_seg + 1)) % 4 == 0 && vr_aligned16(onehot);
  p.png_out = png_out; p.onehot = onehot; p.flag = flag;
  hipLaunchKernelGGL(augment_seg_targets_kernel, dim3((unsigned)vr_cdiv(H, ST_ROWS), B), dim3(256), (size_t)st_lds_bytes(H, W),
                     vr_stream(stream), p);
  VR_LAUNCH_CHECK("augment_seg_targets");
  return VR_OK;
}

extern "C" int vrnet_augment_box_targets_f32(const int* boxes, const int* counts, const vrnet_aug_rec* aug, int B, int max_gt,
                                             int ihm, int iwm, int H, int W, float* targets, int* counts_out, int* flag,
                                             void* stream) {
  VR_CHECK_ARG(boxes && counts && aug && targets && counts_out,
               "augment_box_targets: boxes, counts, aug, targets and counts_out are required");
  VR_CHECK_ARG(fm_shape_ok(B, ihm, iwm, H, W) && max_gt > 0 && max_gt <= (1 << 20),
               "augment_box_targets: bad shape (B %d, max_gt %d, slots %d x %d, canvas %d x %d)", B, max_gt, ihm, iwm, H, W);
  AugBoxArgs p{};
  p.boxes = boxes; p.counts = counts; p.tab = aug;
  p.B = B; p.max_gt = max_gt; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W;
  p.targets = targets; p.counts_out = counts_out; p.flag = flag;
  hipLaunchKernelGGL(augment_box_targets_kernel, dim3(1, B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("augment_box_targets");
  return VR_OK;
}

extern "C" int vrnet_augment_radar_f32(const float* radar, const vrnet_aug_rec* aug, int B, int ihm, int iwm, int H, int W,
                                       float* out, int* flag, void* stream) {
  VR_CHECK_ARG(radar && aug && out && radar != out, "augment_radar: radar, aug and out are required, and out is not the input");
  VR_CHECK_ARG(fm_shape_ok(B, ihm, iwm, H, W) && (long)B * 4 * H * W < (1L << 40), "augment_radar: bad shape (B %d, slots %d x %d, canvas %d x %d)", B, ihm, iwm, H, W);
  AugRadarArgs p{};
  p.radar = radar; p.tab = aug;
  p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W;
  p.out = out; p.flag = flag;
  hipLaunchKernelGGL(augment_radar_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("augment_radar");
  return VR_OK;
}
