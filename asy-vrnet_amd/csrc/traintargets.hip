// The targets of a training batch on the device, from RAW label maps and boxes of mixed sizes: what the `random=False`
// branch of get_random_data (utils/dataloader.py:129-183) and YoloDataset.__getitem__ (:88-105) do on the host per image
// besides the bicubic resize of the frame, which vrnet_letterbox_ragged_u8 (csrc/letterbox.hip) already does.  The
// geometry of image b comes from record b of the vrnet_frame_geom table, clamped on the device (vr_geom_load); grid y is
// the image.  Both results are integers or fp64 arithmetic with one rounding per operation, so they equal the host's
// values bit for bit.
//   seg targets  label (B, ihm, iwm) u8 -> png (B, H, W) int64 and one-hot (B, H, W, ns + 1) f32: Pillow's NEAREST pick
//                inside the window (vr_nearest_indices, the function the letterbox's label output uses), 0 outside, the
//                clamp to the ignore class and the one-hot row of batch_formats_kernel.  A workgroup owns ST_ROWS canvas
//                rows of one image: two of its threads run the two sequential index recurrences into LDS (only when the
//                rows meet the window), every thread then gathers one byte per pixel into LDS and stores the int64 label,
//                and the one-hot rows go out as one flat run of floats -- consecutive lanes cover consecutive addresses,
//                16 B per lane when W (ns + 1) is a multiple of 4, 4 B otherwise.
//   box targets  boxes (B, max_gt, 5) int32 x1, y1, x2, y2, cls in original pixels -> (B, max_gt, 5) f32 cx, cy, w, h, cls on
//                the canvas: data.adjust_boxes (int64 product, IEEE double division, + offset, truncation toward zero; clip;
//                rows thinner than 2 px dropped) and data.boxes_xyxy_to_cxcywh.  One workgroup per image; the kept rows are
//                compacted in input order by a ballot prefix count; rows behind the count are zeroed.
// The row block, the one-hot store, the coordinate map, the clip and keep test and the compaction are augment.h's: the
// augmentation and the Mosaic apply the same rules under their own records.
#include "augment.h"

#pragma clang fp contract(off)

namespace {

struct SegTargetsArgs {
  const unsigned char* label;        // (B, ihm, iwm)
  const vrnet_frame_geom* tab;       // (B)
  int B, ihm, iwm, H, W, ns;
  int vec4;                          // W * (ns + 1) % 4 == 0 and onehot 16-byte aligned: every chunk is whole float4s
  long long* png_out;                // (B, H, W)
  float* onehot;                     // (B, H, W, ns + 1)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void seg_targets_ragged_kernel(const SegTargetsArgs p) {
  extern __shared__ int st_lds[];
  int* xi = st_lds;                  // (W) source column of window column wx
  int* yi = xi + p.W;                // (H) source row of window row wy
  unsigned char* cls = reinterpret_cast<unsigned char*>(yi + p.H);          // (ST_ROWS * W) the clamped label of a pixel
  const int b = blockIdx.y, y0 = blockIdx.x * ST_ROWS;
  const int rows = p.H - y0 < ST_ROWS ? p.H - y0 : ST_ROWS;
  const int npix = rows * p.W, n1 = p.ns + 1;
  bool bad;
  const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  const bool empty = g.ih <= 0 || g.iw <= 0 || g.nw <= 0 || g.nh <= 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  // block-uniform: rows that miss the window are all padding and need no tables
  const bool hit = !empty && y0 < g.dy + g.nh && y0 + rows > g.dy;
  if (hit) {
    if (threadIdx.x == 0) vr_nearest_indices(g.iw, g.nw, xi);
    if (threadIdx.x == 64) vr_nearest_indices(g.ih, g.nh, yi);             // another wave: the two recurrences run side by side
  }
  __syncthreads();
  const unsigned char* src = p.label + (long)b * p.ihm * p.iwm;
  long long* png = p.png_out + ((long)b * p.H + y0) * p.W;
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int r = i / p.W;
    const int wx = i - r * p.W - g.dx, wy = y0 + r - g.dy;
    int lab = 0;
    if (hit && wx >= 0 && wx < g.nw && wy >= 0 && wy < g.nh) {
      const int sx = xi[wx], sy = yi[wy];
      if (sx >= 0 && sx < g.iw && sy >= 0 && sy < g.ih) lab = src[(long)sy * p.iwm + sx];   // ImagingScaleAffine leaves the rest unset
    }
    if (lab >= p.ns) lab = p.ns;
    cls[i] = (unsigned char)lab;
    png[i] = lab;
  }
  __syncthreads();
  st_store_onehot(cls, p.onehot + ((long)b * p.H + y0) * p.W * n1, npix, n1, p.vec4);
}

struct BoxTargetsArgs {
  const int* boxes;                  // (B, max_gt, 5)
  const int* counts;                 // (B)
  const vrnet_frame_geom* tab;       // (B)
  int B, max_gt, ihm, iwm, H, W;
  float* targets;                    // (B, max_gt, 5)
  int* counts_out;                   // (B)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void box_targets_ragged_kernel(const BoxTargetsArgs p) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y;
  bool bad;
  const vrnet_frame_geom g = vr_geom_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  const bool empty = g.ih <= 0 || g.iw <= 0 || g.nw <= 0 || g.nh <= 0;
  const int given = p.counts[b];
  const int n = empty ? 0 : vr_clampi(given, 0, p.max_gt);
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
      keep = box_clip_keep(x1, y1, x2, y2, p.W, p.H);
    }
    const int at = box_compact_slot(keep, base, s_wave);
    if (keep) box_store_cxcywh(out + (long)at * 5, x1, y1, x2, y2, c);      // at <= i < max_gt: compaction never moves a row up
    __syncthreads();                 // s_wave is rewritten by the next chunk
  }
  box_zero_tail(base, p.max_gt, out);
  if (threadIdx.x == 0) p.counts_out[b] = base;
}

}  // namespace

extern "C" int vrnet_seg_targets_ragged_u8(const unsigned char* label, const vrnet_frame_geom* geom, int B, int ihm, int iwm,
                                           int H, int W, int num_classes_seg, long long* png_out, float* onehot, int* flag,
                                           void* stream) {
  VR_CHECK_ARG(label && geom && png_out && onehot, "seg_targets_ragged: label, geom, png_out and onehot are required");
  VR_CHECK_ARG(B > 0 && B < 65536 && ihm > 0 && iwm > 0 && H > 0 && W > 0,
               "seg_targets_ragged: bad shape (B %d, slots %d x %d, canvas %d x %d)", B, ihm, iwm, H, W);
  VR_CHECK_ARG(num_classes_seg > 0 && num_classes_seg < 255, "seg_targets_ragged: 0 < num_classes_seg < 255, got %d",
               num_classes_seg);
  VR_CHECK_ARG(st_lds_bytes(H, W) <= ST_LDS_MAX, "seg_targets_ragged: a %d x %d canvas needs %ld bytes of LDS, above %ld", H, W,
               st_lds_bytes(H, W), ST_LDS_MAX);
  VR_CHECK_ARG((long)B * ihm * iwm < (1L << 31) && (long)B * H * W * (num_classes_seg + 1) < (1L << 40) &&
                   (long)ST_ROWS * W * (num_classes_seg + 1) < (1L << 31),
               "seg_targets_ragged: batch too large");
  SegTargetsArgs p{};
  p.label = label; p.tab = geom;
  p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.ns = num_classes_seg;
  p.vec4 = ((long)W * (num_classes_seg + 1)) % 4 == 0 && vr_aligned16(onehot);
  p.png_out = png_out; p.onehot = onehot; p.flag = flag;
  hipLaunchKernelGGL(seg_targets_ragged_kernel, dim3((unsigned)vr_cdiv(H, ST_ROWS), B), dim3(256), (size_t)st_lds_bytes(H, W),
                     vr_stream(stream), p);
  VR_LAUNCH_CHECK("seg_targets_ragged");
  return VR_OK;
}

extern "C" int vrnet_box_targets_ragged_f32(const int* boxes, const int* counts, const vrnet_frame_geom* geom, int B,
                                            int max_gt, int ihm, int iwm, int H, int W, float* targets, int* counts_out,
                                            int* flag, void* stream) {
  VR_CHECK_ARG(boxes && counts && geom && targets && counts_out,
               "box_targets_ragged: boxes, counts, geom, targets and counts_out are required");
  VR_CHECK_ARG(B > 0 && B < 65536 && max_gt > 0 && max_gt <= (1 << 20) && ihm > 0 && iwm > 0 && H > 0 && W > 0 &&
                   H <= (1 << 24) && W <= (1 << 24),
               "box_targets_ragged: bad shape (B %d, max_gt %d, slots %d x %d, canvas %d x %d)", B, max_gt, ihm, iwm, H, W);
  BoxTargetsArgs p{};
  p.boxes = boxes; p.counts = counts; p.tab = geom;
  p.B = B; p.max_gt = max_gt; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W;
  p.targets = targets; p.counts_out = counts_out; p.flag = flag;
  hipLaunchKernelGGL(box_targets_ragged_kernel, dim3(1, B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("box_targets_ragged");
  return VR_OK;
}
