// Mosaic, the four-tiles-into-one-canvas augmentation of utils/dataloader.py:251-426 (get_random_data_with_Mosaic,
// merge_bboxes), on the device and from raw bytes, extended to the label map and the radar map by this project's own rule
// (data.mosaic_sample).  Nothing here is random: the host draws one vrnet_mosaic_rec per OUTPUT image (data.mosaic_params) and
// these kernels apply it, so they equal the host functions of data.py bit for bit.  What they share with the single-image
// augmentation is in augment.h and resample.h.
// The canvas is cut at (cutx, cuty) into four quadrants, one per tile (dataloader.py:393-397): tile 0 x < cutx, y < cuty;
// tile 1 x < cutx, y >= cuty; tile 2 x >= cutx, y >= cuty; tile 3 x >= cutx, y < cuty.  A tile is a source frame (slot src of
// the S slots; -1: no tile) mirrored left-right when flip is set, resized to nw x nh and pasted at (dx, dy); only what falls
// into its quadrant shows.  Differences to augment.hip:
//   the flip mirrors the SOURCE before the resize (:328-344), not the canvas: the kernels mirror the source column they read
//     and keep the tables of the unflipped axis.  Pillow's NEAREST recurrence is not mirror-symmetric, so for the label map
//     this is not the same as mirroring the window index
//   tables, the horizontal result and the nearest indices are indexed by CANVAS column / row.  Tiles 0 and 3 (the top half)
//     share no column and tiles 1 and 2 (the bottom half) share none, so two column sets of W entries serve four tiles;
//     likewise two row sets of H entries for the left (0, 1) and the right (3, 2) side: twice the single-image workspace
//   the four tile heads are loaded wave-uniformly and selected per lane by quadrant: a wave that straddles a cut sees two
// Kernels (grid y = OUTPUT image; mos_load clamps the record so that no access leaves a slot, the canvas or the workspace;
// if ANY tile had to be clamped the whole output image is what an empty record gives and VR_FLAG_GEOMETRY is set):
//   tables      bounds and taps of the columns and rows each tile shows inside its quadrant, one thread each
//   horizontal  (ih, iw, 3) of the tile's source -> (ih, its visible columns, 3) in the workspace; skipped when nw == iw
//   vertical    one thread per canvas pixel: quadrant select, vertical taps (a copy when nh == ih), paste, colour,
//               normalise_store; consecutive lanes store consecutive x
//   seg         the NEAREST pick per tile, on the mirrored source column when flipped
//   boxes       per tile and row: flip, map, clip, keep, merge_bboxes at the cut, keep again; compacted across the sources
//   radar       an integer gather of the tile's stored map
//   radar points (init, points, resolve)  the radar input from the POINTS of the sources instead: every point of a tile's
//               source is projected into the tile's window once and competes for the pixels of the tile's quadrant
#include "augment.h"
#include "radarpoint.h"

#pragma clang fp contract(off)

extern "C" {
/* include/vrnet_hip.h: one tile of a Mosaic record (48 bytes) and the record per output image (976 bytes). */
typedef struct vrnet_mosaic_tile {
  int src;                           /* the source slot, 0 .. S - 1; -1: no tile */
  int ih, iw;                        /* that source's own size inside its (ihm, iwm) slot */
  int nw, nh, dx, dy;                /* the resized tile and where it is pasted; may leave the canvas on every side */
  int flip;                          /* != 0: mirror the SOURCE left-right before the resize */
  int lb_nw, lb_nh, lb_dx, lb_dy;    /* data.letterbox_geometry of the source: the window its stored radar map is aligned with */
} vrnet_mosaic_tile;
typedef struct vrnet_mosaic_rec {
  int cutx, cuty;                    /* 0 <= cutx <= W, 0 <= cuty <= H */
  int color, reserved;               /* != 0: run the colour stage over the finished canvas; 0 */
  vrnet_mosaic_tile tile[4];         /* in the reference's tile order */
  unsigned char lut[3][256];         /* hue, saturation, value tables of the colour stage */
} vrnet_mosaic_rec;
/* include/vrnet_hip.h: what vrnet_mosaic_radar_points_f32 knows of a source beside the Mosaic record (56 bytes). */
typedef struct vrnet_radar_source {
  int count, reserved;               /* the source's points; 0 */
  float P[12];                       /* (3, 4) row-major: (x, y, z, 1) -> homogeneous continuous pixel coordinates of the source */
} vrnet_radar_source;
}
static_assert(sizeof(vrnet_radar_source) == 56 && alignof(vrnet_radar_source) == 4, "vrnet_radar_source layout");
static_assert(sizeof(vrnet_mosaic_tile) == 48 && sizeof(vrnet_mosaic_rec) == 976 && alignof(vrnet_mosaic_rec) == 4,
              "vrnet_mosaic_rec layout");

namespace {

constexpr int MOS_HEAD_INTS = 4, MOS_TILE_INTS = 12;
constexpr int MOS_LUT_INTS = MOS_HEAD_INTS + 4 * MOS_TILE_INTS;      // the tables sit at byte 208: 4-byte aligned words

// a tile's fields as an array, so that the per-lane pick below is sixteen selects
enum { T_SRC, T_IH, T_IW, T_NW, T_NH, T_DX, T_DY, T_FLIP, T_LNW, T_LNH, T_LDX, T_LDY, T_XA, T_XB, T_YA, T_YB, T_FIELDS };

struct MosTile {
  int v[T_FIELDS];                   // the head, clamped; [xa, xb) x [ya, yb): the canvas pixels the tile shows (empty: none)
};

struct MosRec {
  int cutx, cuty, color;
  MosTile t[4];
};

__device__ __forceinline__ int mos_side(int t) { return t >= 2; }                  // 1: right of the cut
__device__ __forceinline__ int mos_half(int t) { return t == 1 || t == 2; }        // 1: below the cut
__device__ __forceinline__ int mos_tile_of(int side, int half) { return side ? (half ? 2 : 3) : (half ? 1 : 0); }

// Record b, clamped, tile by tile as aug_load clamps a single-image record: src in -1 .. S - 1; 0 <= ih <= ihm, 0 <= iw <= iwm;
// 0 <= nw, nh <= 2 max(W, H); -nw <= dx <= W, -nh <= dy <= H; the letterbox window inside the canvas; the cut inside the
// canvas.  A tile with src == -1 is absent and the rest of its head is not looked at.  bad: something was clamped, or a
// size or window of a present tile is not positive.  A bad record is not applied in part: every tile is then absent and
// the colour stage off, which is what an empty record gives.  b is the block's image, so all loads are wave-uniform.
__device__ __forceinline__ MosRec mos_load(const vrnet_mosaic_rec* tab, int b, int S, int ihm, int iwm, int H, int W, bool& bad) {
  const int* r = reinterpret_cast<const int*>(tab + b);
  MosRec g;
  g.cutx = vr_clampi(r[0], 0, W);
  g.cuty = vr_clampi(r[1], 0, H);
  g.color = r[2] != 0;
  bad = g.cutx != r[0] || g.cuty != r[1];
  const int lim = 2 * (W > H ? W : H);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int* h = r + MOS_HEAD_INTS + t * MOS_TILE_INTS;
    int* v = g.t[t].v;
    v[T_SRC] = vr_clampi(h[0], -1, S - 1);
    v[T_IH] = vr_clampi(h[1], 0, ihm);
    v[T_IW] = vr_clampi(h[2], 0, iwm);
    v[T_NW] = vr_clampi(h[3], 0, lim);
    v[T_NH] = vr_clampi(h[4], 0, lim);
    v[T_DX] = vr_clampi(h[5], -v[T_NW], W);
    v[T_DY] = vr_clampi(h[6], -v[T_NH], H);
    v[T_FLIP] = h[7] != 0;
    v[T_LNW] = vr_clampi(h[8], 0, W);
    v[T_LNH] = vr_clampi(h[9], 0, H);
    v[T_LDX] = vr_clampi(h[10], 0, W - v[T_LNW]);
    v[T_LDY] = vr_clampi(h[11], 0, H - v[T_LNH]);
    if (h[0] == -1) continue;
    bad = bad || v[T_SRC] != h[0] || v[T_IH] != h[1] || v[T_IW] != h[2] || v[T_NW] != h[3] || v[T_NH] != h[4] || v[T_DX] != h[5] ||
          v[T_DY] != h[6] || v[T_LNW] != h[8] || v[T_LNH] != h[9] || v[T_LDX] != h[10] || v[T_LDY] != h[11] || h[1] <= 0 ||
          h[2] <= 0 || h[3] <= 0 || h[4] <= 0 || h[8] <= 0 || h[9] <= 0;
  }
  if (bad) g.color = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    int* v = g.t[t].v;
    if (bad) v[T_SRC] = -1;
    // the quadrant, and the part of the window inside it
    const int qx0 = mos_side(t) ? g.cutx : 0, qx1 = mos_side(t) ? W : g.cutx;
    const int qy0 = mos_half(t) ? g.cuty : 0, qy1 = mos_half(t) ? H : g.cuty;
    const int xa = v[T_DX] > qx0 ? v[T_DX] : qx0, xe = v[T_DX] + v[T_NW] < qx1 ? v[T_DX] + v[T_NW] : qx1;
    const int ya = v[T_DY] > qy0 ? v[T_DY] : qy0, ye = v[T_DY] + v[T_NH] < qy1 ? v[T_DY] + v[T_NH] : qy1;
    const bool none = v[T_SRC] < 0 || xe <= xa || ye <= ya;         // 0 <= xa < xe <= W, 0 <= ya < ye <= H otherwise
    v[T_XA] = none ? 0 : xa;
    v[T_XB] = none ? 0 : xe;
    v[T_YA] = none ? 0 : ya;
    v[T_YB] = none ? 0 : ye;
  }
  return g;
}

// tile q of the record, q per lane
__device__ __forceinline__ MosTile mos_pick(const MosRec& g, int q) {
  MosTile r;
#pragma unroll
  for (int k = 0; k < T_FIELDS; ++k) r.v[k] = q == 0 ? g.t[0].v[k] : (q == 1 ? g.t[1].v[k] : (q == 2 ? g.t[2].v[k] : g.t[3].v[k]));
  return r;
}

__device__ __forceinline__ bool mos_shows(const MosTile& t, int x, int y) {
  return x >= t.v[T_XA] && x < t.v[T_XB] && y >= t.v[T_YA] && y < t.v[T_YB];
}

struct MosFramesArgs {
  const unsigned char* img;          // (S, ihm, iwm, 3)
  const vrnet_mosaic_rec* tab;       // (B)
  int S, B, ihm, iwm, H, W, cap;     // cap: taps per table entry
  long slot;                         // ints of one table set
  int* tables;                       // (B, 2) sets
  unsigned char* mid;                // (B, 2, ihm, W, 3): the horizontal pass's result of the top and the bottom half
  unsigned char* canvas;             // (B, H, W, 3) or null
  float* images;                     // (B, 3, H, W) or null
  int* flag;                         // or null
};

struct MosTables {
  int *hb, *hk, *vb, *vk;            // taps of canvas column x: hk[t * W + x]; of canvas row y: vk[t * H + y]
};

// set s of image b: the columns of half s (tiles 0 | 3, or 1 | 2) and the rows of side s (tiles 0 / 1, or 3 / 2)
__device__ __forceinline__ MosTables mos_tables(const MosFramesArgs& p, int b, int s) {
  MosTables m;
  int* t = p.tables + ((long)b * 2 + s) * p.slot;
  m.hb = t; t += 2L * p.W;
  m.hk = t; t += (long)p.W * p.cap;
  m.vb = t; t += 2L * p.H;
  m.vk = t;
  return m;
}

__global__ __launch_bounds__(256) void mosaic_tables_kernel(const MosFramesArgs p) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x, n = p.W + p.H;
  bool bad;
  const MosRec g = mos_load(p.tab, b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  if (e == 0 && p.flag) {            // a clamped record, or taps beyond the capacity (bicubic_taps_at then truncates them)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int* v = g.t[t].v;
      if (v[T_SRC] >= 0)
        bad = bad || (v[T_NW] != v[T_IW] && lb_ksize(v[T_IW], v[T_NW]) > p.cap) || (v[T_NH] != v[T_IH] && lb_ksize(v[T_IH], v[T_NH]) > p.cap);
    }
    if (bad) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  }
  if (e >= 2 * n) return;
  const int s = e >= n, i = e - s * n;
  const MosTables m = mos_tables(p, b, s);
  if (i < p.W) {                     // column i of half s
    const MosTile t = mos_pick(g, mos_tile_of(i >= g.cutx, s));
    if (i >= t.v[T_XA] && i < t.v[T_XB] && t.v[T_NW] != t.v[T_IW])
      bicubic_taps_at(i - t.v[T_DX], t.v[T_IW], t.v[T_NW], p.cap, m.hb, m.hk, i, p.W);
  } else {                           // row y of side s
    const int y = i - p.W;
    const MosTile t = mos_pick(g, mos_tile_of(s, y >= g.cuty));
    if (y >= t.v[T_YA] && y < t.v[T_YB] && t.v[T_NH] != t.v[T_IH])
      bicubic_taps_at(y - t.v[T_DY], t.v[T_IH], t.v[T_NH], p.cap, m.vb, m.vk, y, p.H);
  }
}

__global__ __launch_bounds__(256) void mosaic_horizontal_kernel(const MosFramesArgs p) {
  const int b = blockIdx.y;
  bool bad;
  const MosRec g = mos_load(p.tab, b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  const long e = (long)blockIdx.x * 256 + threadIdx.x, per = (long)p.ihm * p.W;
  if (e >= 2 * per) return;
  const int half = e >= per;
  const long i = e - half * per;
  const int row = (int)(i / p.W), x = (int)(i - (long)row * p.W);
  const MosTile t = mos_pick(g, mos_tile_of(x >= g.cutx, half));
  // a tile that shows nothing here has xa == xb; one with nw == iw skips the pass, as Pillow does
  if (x < t.v[T_XA] || x >= t.v[T_XB] || row >= t.v[T_IH] || t.v[T_NW] == t.v[T_IW]) return;
  const MosTables m = mos_tables(p, b, half);
  const int xmin = m.hb[2 * x], n = m.hb[2 * x + 1];            // xmin + n <= iw: inside the slot's row
  const unsigned char* src = p.img + ((long)t.v[T_SRC] * p.ihm + row) * p.iwm * 3;
  // the flipped source: column c of it is column iw - 1 - c of the slot
  const int first = t.v[T_FLIP] ? t.v[T_IW] - 1 - xmin : xmin, step = t.v[T_FLIP] ? -3 : 3;
  resample_taps3(src + (long)first * 3, step, m.hk + x, p.W, n, p.mid + ((((long)b * 2 + half) * p.ihm + row) * p.W + x) * 3);
}

__global__ __launch_bounds__(256) void mosaic_vertical_paste_kernel(const MosFramesArgs p) {
  __shared__ ColorLds c;
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const MosRec g = mos_load(p.tab, (int)b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  if (g.color)                       // block-uniform
    color_lds_fill(c, reinterpret_cast<const unsigned*>(reinterpret_cast<const int*>(p.tab + b) + MOS_LUT_INTS));
  if (r >= HW) return;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const int side = x >= g.cutx, half = y >= g.cuty;
  const MosTile t = mos_pick(g, mos_tile_of(side, half));
  unsigned char v[3] = {128, 128, 128};
  if (mos_shows(t, x, y)) {
    const int wx = x - t.v[T_DX], wy = y - t.v[T_DY];
    // the horizontal result: the workspace (rows of W canvas columns), or the source's own slot when that pass was skipped
    const bool resized = t.v[T_NW] != t.v[T_IW];
    const unsigned char* src = resized ? p.mid + ((b * 2 + half) * p.ihm * p.W + x) * 3
                                       : p.img + ((long)t.v[T_SRC] * p.ihm * p.iwm + (t.v[T_FLIP] ? t.v[T_IW] - 1 - wx : wx)) * 3;
    const long rs = (resized ? (long)p.W : (long)p.iwm) * 3;
    if (t.v[T_NH] != t.v[T_IH]) {
      const MosTables m = mos_tables(p, (int)b, side);
      const int ymin = m.vb[2 * y], n = m.vb[2 * y + 1];
      resample_taps3(src + ymin * rs, rs, m.vk + y, p.H, n, v);
    } else {
      src += wy * rs;
      v[0] = src[0];
      v[1] = src[1];
      v[2] = src[2];
    }
  }
  paste_store(c, g.color, v, p.canvas, p.images, b, HW, r);
}

// ---- the segmentation targets ------------------------------------------------------------------------------------------------
struct MosSegArgs {
  const unsigned char* label;        // (S, ihm, iwm)
  const vrnet_mosaic_rec* tab;       // (B)
  int S, B, ihm, iwm, H, W, ns;
  int vec4;                          // W * (ns + 1) % 4 == 0 and onehot 16-byte aligned: every chunk is whole float4s
  long long* png_out;                // (B, H, W)
  float* onehot;                     // (B, H, W, ns + 1)
  int* flag;                         // or null
};

__host__ __device__ inline long mos_st_lds_bytes(int H, int W) { return 2 * ((long)W + H) * (long)sizeof(int) + (long)ST_ROWS * W; }

__global__ __launch_bounds__(256) void mosaic_seg_targets_kernel(const MosSegArgs p) {
  extern __shared__ int st_lds[];
  int* xi = st_lds;                  // (2, W) by half: the column of the (flipped) source that canvas column x shows
  int* yi = xi + 2 * p.W;            // (2, H) by side: the source row that canvas row y shows
  unsigned char* cls = reinterpret_cast<unsigned char*>(yi + 2 * p.H);      // (ST_ROWS * W) the clamped label of a pixel
  const int b = blockIdx.y, y0 = blockIdx.x * ST_ROWS;
  const int rows = p.H - y0 < ST_ROWS ? p.H - y0 : ST_ROWS;
  const int npix = rows * p.W, n1 = p.ns + 1;
  bool bad;
  const MosRec g = mos_load(p.tab, b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  // eight serial recurrences, columns and rows of the four tiles, on eight lanes two to a wave: each runs from window index
  // 0 to the last one the tile shows in these rows, and keeps what it shows
  if ((threadIdx.x & 31) == 0) {
    const int job = threadIdx.x >> 5;
    const MosTile t = mos_pick(g, job & 3);
    const int ya = t.v[T_YA] > y0 ? t.v[T_YA] : y0, yb = t.v[T_YB] < y0 + rows ? t.v[T_YB] : y0 + rows;
    if (yb > ya) {                   // the tile shows something in this block's rows
      if (job < 4)
        vr_nearest_indices_from(t.v[T_IW], t.v[T_NW], t.v[T_XA] - t.v[T_DX], t.v[T_XB] - t.v[T_XA],
                                xi + mos_half(job & 3) * p.W + t.v[T_XA]);
      else
        vr_nearest_indices_from(t.v[T_IH], t.v[T_NH], ya - t.v[T_DY], yb - ya, yi + mos_side(job & 3) * p.H + ya);
    }
  }
  __syncthreads();
  long long* png = p.png_out + ((long)b * p.H + y0) * p.W;
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int r = i / p.W, x = i - r * p.W, y = y0 + r;
    const int side = x >= g.cutx, half = y >= g.cuty;
    const MosTile t = mos_pick(g, mos_tile_of(side, half));
    int lab = 0;
    if (mos_shows(t, x, y)) {
      const int sx = xi[half * p.W + x], sy = yi[side * p.H + y];
      if (sx >= 0 && sx < t.v[T_IW] && sy >= 0 && sy < t.v[T_IH])      // ImagingScaleAffine leaves the rest unset
        lab = p.label[((long)t.v[T_SRC] * p.ihm + sy) * p.iwm + (t.v[T_FLIP] ? t.v[T_IW] - 1 - sx : sx)];
    }
    if (lab >= p.ns) lab = p.ns;
    cls[i] = (unsigned char)lab;
    png[i] = lab;
  }
  __syncthreads();
  st_store_onehot(cls, p.onehot + ((long)b * p.H + y0) * p.W * n1, npix, n1, p.vec4);
}

// ---- the box targets ---------------------------------------------------------------------------------------------------------
struct MosBoxArgs {
  const int* boxes;                  // (S, max_gt, 5)
  const int* counts;                 // (S)
  const vrnet_mosaic_rec* tab;       // (B)
  int S, B, max_gt, ihm, iwm, H, W;
  float* targets;                    // (B, max_gt, 5)
  int* counts_out;                   // (B)
  int* flag;                         // or null
};

// merge_bboxes (dataloader.py:251-295) for one box of tile t, verbatim: false when the box is skipped
__device__ __forceinline__ bool mos_merge(int t, long long& x1, long long& y1, long long& x2, long long& y2, int cutx, int cuty) {
  if (t == 0) {
    if (y1 > cuty || x1 > cutx) return false;
    if (y2 >= cuty && y1 <= cuty) y2 = cuty;
    if (x2 >= cutx && x1 <= cutx) x2 = cutx;
  } else if (t == 1) {
    if (y2 < cuty || x1 > cutx) return false;
    if (y2 >= cuty && y1 <= cuty) y1 = cuty;
    if (x2 >= cutx && x1 <= cutx) x2 = cutx;
  } else if (t == 2) {
    if (y2 < cuty || x2 < cutx) return false;
    if (y2 >= cuty && y1 <= cuty) y1 = cuty;
    if (x2 >= cutx && x1 <= cutx) x1 = cutx;
  } else {
    if (y1 > cuty || x2 < cutx) return false;
    if (y2 >= cuty && y1 <= cuty) y2 = cuty;
    if (x2 >= cutx && x1 <= cutx) x1 = cutx;
  }
  return true;
}

__global__ __launch_bounds__(256) void mosaic_box_targets_kernel(const MosBoxArgs p) {
  __shared__ int s_wave[4];
  const int b = blockIdx.y;
  bool bad;
  const MosRec g = mos_load(p.tab, b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  float* out = p.targets + (long)b * p.max_gt * 5;
  int bits = bad ? VR_FLAG_GEOMETRY : 0;
  int base = 0;                      // rows kept so far, in tile-then-row order: the same in every thread
  for (int t = 0; t < 4; ++t) {      // uniform
    const int* v = g.t[t].v;
    if (v[T_SRC] < 0) continue;
    const int given = p.counts[v[T_SRC]];
    const int n = vr_clampi(given, 0, p.max_gt);
    if (given < 0 || given > p.max_gt) bits |= VR_FLAG_BOX_COUNT;
    const int* rows = p.boxes + (long)v[T_SRC] * p.max_gt * 5;
    for (int start = 0; start < n; start += 256) {
      const int i = start + threadIdx.x;
      bool keep = false;
      long long x1 = 0, y1 = 0, x2 = 0, y2 = 0;
      int c = 0;
      if (i < n) {
        const int* r = rows + (long)i * 5;
        x1 = r[0];
        x2 = r[2];
        c = r[4];
        if (v[T_FLIP]) {             // box[:, [0, 2]] = iw - box[:, [2, 0]] (dataloader.py:331), on the integer array
          const long long f = v[T_IW] - x2;
          x2 = v[T_IW] - x1;
          x1 = f;
        }
        x1 = map_coord(x1, v[T_NW], v[T_IW], v[T_DX]);
        y1 = map_coord(r[1], v[T_NH], v[T_IH], v[T_DY]);
        x2 = map_coord(x2, v[T_NW], v[T_IW], v[T_DX]);
        y2 = map_coord(r[3], v[T_NH], v[T_IH], v[T_DY]);
        keep = box_clip_keep(x1, y1, x2, y2, p.W, p.H);
        keep = keep && mos_merge(t, x1, y1, x2, y2, g.cutx, g.cuty);
        keep = keep && x2 - x1 > 1 && y2 - y1 > 1;           // what the cut reduced to a line or less is dropped
      }
      const int at = box_compact_slot(keep, base, s_wave);
      // four sources can keep more than max_gt rows between them: the first max_gt stay.  box_store_cxcywh (augment.h),
      // written out: the call gave this kernel other registers and another instruction schedule
      if (keep && at < p.max_gt) {
        const double w = (double)(x2 - x1), h = (double)(y2 - y1);
        float* o = out + (long)at * 5;
        o[0] = (float)((double)x1 + w / 2);
        o[1] = (float)((double)y1 + h / 2);
        o[2] = (float)w;
        o[3] = (float)h;
        o[4] = (float)c;
      }
      __syncthreads();               // s_wave is rewritten by the next chunk
    }
  }
  if (base > p.max_gt) {
    bits |= VR_FLAG_BOX_COUNT;
    base = p.max_gt;
  }
  box_zero_tail(base, p.max_gt, out);
  if (threadIdx.x == 0) {
    p.counts_out[b] = base;
    if (bits && p.flag) atomicOr(p.flag, bits);
  }
}

// ---- the radar map -----------------------------------------------------------------------------------------------------------
struct MosRadarArgs {
  const float* radar;                // (S, 4, H, W): each aligned with the letterbox window of its source
  const vrnet_mosaic_rec* tab;       // (B)
  int S, B, ihm, iwm, H, W;          // ihm, iwm: only to judge the record as the other three kernels do
  float* out;                        // (B, 4, H, W)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void mosaic_radar_kernel(const MosRadarArgs p) {
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const MosRec g = mos_load(p.tab, (int)b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  if (r >= HW) return;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const MosTile t = mos_pick(g, mos_tile_of(x >= g.cutx, y >= g.cuty));
  const bool inside = mos_shows(t, x, y);
  long at = 0;
  if (inside) {
    const int wy = y - t.v[T_DY], wx = t.v[T_FLIP] ? t.v[T_NW] - 1 - (x - t.v[T_DX]) : x - t.v[T_DX];
    at = radar_pick((long)t.v[T_SRC] * 4 * HW, wx, wy, t.v[T_NW], t.v[T_NH], t.v[T_LNW], t.v[T_LNH], t.v[T_LDX], t.v[T_LDY], p.W);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) p.out[(b * 4 + c) * HW + r] = inside ? p.radar[at + c * HW] : 0.f;
}

// ---- the radar map from the sources' points --------------------------------------------------------------------------------
// data.mosaic_radar_map: tile t of output image b is data.radar_map of its source's points under the tile's window, cut to
// the tile's quadrant.  A mirrored tile puts window pixel ix at canvas column dx + nw - 1 - ix (the SOURCE is mirrored, the
// window stays where it is).  [xa, xb) x [ya, yb) of mos_load is the window cut by the quadrant, which lies inside the canvas:
// the footprint of a point is clipped to it, so a key plane only ever holds candidates of the tile that owns the pixel and
// the resolve pass reads the winner's features from that tile's source.
struct MosPointsArgs {
  const float* points;               // (S, max_points, 7)
  const vrnet_radar_source* src;     // (S)
  const vrnet_mosaic_rec* tab;       // (B)
  int S, B, max_points, ihm, iwm, H, W, radius;
  float min_depth;
  unsigned long long* keys;          // (B, H, W)
  float* out;                        // (B, 4, H, W)
  int* flag;                         // or null
};

__global__ __launch_bounds__(256) void mosaic_radar_points_init_kernel(unsigned long long* keys, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = RM_EMPTY;
}

// grid (point chunks, 4 tiles, B output images): the record, the tile and the source's entry are the same in every lane
__global__ __launch_bounds__(256) void mosaic_radar_points_kernel(const MosPointsArgs p) {
  const int b = blockIdx.z, q = blockIdx.y;
  bool bad;
  const MosRec g = mos_load(p.tab, b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  const MosTile t = mos_pick(g, q);
  const int src = t.v[T_SRC];                                   // -1 .. S - 1 (mos_load); -1 for every tile of a bad record
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (first && q == 0 && bad && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  if (src < 0) return;
  const vrnet_radar_source* s = p.src + src;
  const int given = s->count, count = vr_clampi(given, 0, p.max_points);
  if (first && count != given && p.flag) atomicOr(p.flag, VR_FLAG_POINT_COUNT);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count || t.v[T_XA] >= t.v[T_XB] || t.v[T_YA] >= t.v[T_YB]) return;
  int ix, iy;
  float hw;
  if (!rm_project(s->P, p.points + ((long)src * p.max_points + i) * RM_POINT_FLOATS, p.min_depth, t.v[T_IH], t.v[T_IW], t.v[T_NW],
                  t.v[T_NH], ix, iy, hw))
    return;
  // the centre on the canvas, 64-bit as in radarmap.hip; the covered pixels are inside [xa, xb) x [ya, yb), hence the canvas
  const long long cx = (long long)t.v[T_DX] + (t.v[T_FLIP] ? t.v[T_NW] - 1 - ix : ix), cy = (long long)t.v[T_DY] + iy;
  long long x0 = cx - p.radius, x1 = cx + p.radius, y0 = cy - p.radius, y1 = cy + p.radius;
  x0 = x0 < t.v[T_XA] ? t.v[T_XA] : x0;
  y0 = y0 < t.v[T_YA] ? t.v[T_YA] : y0;
  x1 = x1 > t.v[T_XB] - 1 ? t.v[T_XB] - 1 : x1;
  y1 = y1 > t.v[T_YB] - 1 ? t.v[T_YB] - 1 : y1;
  if (x0 > x1 || y0 > y1) return;
  const unsigned long long key = rm_key(hw, i);
  unsigned long long* plane = p.keys + (long)b * p.H * p.W;
  for (int yy = (int)y0; yy <= (int)y1; ++yy)
    for (int xx = (int)x0; xx <= (int)x1; ++xx) atomicMin(plane + (long)yy * p.W + xx, key);
}

__global__ __launch_bounds__(256) void mosaic_radar_points_resolve_kernel(const MosPointsArgs p) {
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  bool bad;
  const MosRec g = mos_load(p.tab, (int)b, p.S, p.ihm, p.iwm, p.H, p.W, bad);
  if (r >= HW) return;
  const int y = (int)(r / p.W), x = (int)(r - (long)y * p.W);
  const MosTile t = mos_pick(g, mos_tile_of(x >= g.cutx, y >= g.cuty));
  const unsigned long long key = p.keys[b * HW + r];
  const unsigned idx = (unsigned)key;
  unsigned f[4] = {0u, 0u, 0u, 0u};
  // a key is only ever written inside what its tile shows, by a point below its source's count
  if (key != RM_EMPTY && idx < (unsigned)p.max_points && mos_shows(t, x, y)) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p.points) + ((long)t.v[T_SRC] * p.max_points + idx) * RM_POINT_FLOATS + 3;
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = q[c];
  }
  unsigned* out = reinterpret_cast<unsigned*>(p.out);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[(b * 4 + c) * HW + r] = f[c];
}

long mos_points_bytes(int B, int H, int W) { return (((long)B * H * W * 8) + 255) & ~255L; }

bool mos_shape_ok(int S, int B, int ihm, int iwm, int H, int W) {
  return S > 0 && S < (1 << 20) && fm_shape_ok(B, ihm, iwm, H, W) && (long)S * ihm * iwm < (1L << 31) &&
         (long)B * H * W < (1L << 31);
}

}  // namespace

// two table sets and two horizontal results per output image
extern "C" long vrnet_mosaic_workspace_bytes(int B, int ihm, int iwm, int H, int W, int max_taps) {
  (void)iwm;
  return fm_workspace_bytes(2L * B, ihm, H, W, max_taps);
}

extern "C" int vrnet_mosaic_frames_u8(const unsigned char* img, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm,
                                      int H, int W, int max_taps, unsigned char* canvas, float* images, int* flag,
                                      void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(img && mosaic && mos_shape_ok(S, B, ihm, iwm, H, W) && max_taps >= 5 && max_taps <= 4096,
               "mosaic_frames: bad shape (S %d, B %d, slots %d x %d, canvas %d x %d, max_taps %d)", S, B, ihm, iwm, H, W, max_taps);
  VR_CHECK_ARG(canvas || images, "mosaic_frames: no output requested");
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(mosaic) & 7) == 0, "mosaic_frames: the record table must be 8-byte aligned");
  VR_CHECK_ARG(2L * B * ihm * W < (1L << 31) && 2L * B * lb_ragged_slot_ints(H, W, max_taps) < (1L << 31),
               "mosaic_frames: batch too large");
  MosFramesArgs p{};
  if (!fm_split_workspace("mosaic_frames", workspace, workspace_bytes, 2L * B, ihm, H, W, max_taps, p.tables, p.mid)) return VR_ERR_WORKSPACE;
  p.img = img; p.tab = mosaic;
  p.S = S; p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.cap = max_taps;
  p.slot = lb_ragged_slot_ints(H, W, max_taps);
  p.canvas = canvas; p.images = images; p.flag = flag;
  hipStream_t st = vr_stream(stream);
  hipLaunchKernelGGL(mosaic_tables_kernel, dim3((unsigned)vr_cdiv(2L * (W + H), 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(mosaic_horizontal_kernel, dim3((unsigned)vr_cdiv(2L * ihm * W, 256), B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(mosaic_vertical_paste_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("mosaic_frames");
  return VR_OK;
}

extern "C" int vrnet_mosaic_seg_targets_u8(const unsigned char* label, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm,
                                           int iwm, int H, int W, int num_classes_seg, long long* png_out, float* onehot,
                                           int* flag, void* stream) {
  VR_CHECK_ARG(label && mosaic && png_out && onehot, "mosaic_seg_targets: label, mosaic, png_out and onehot are required");
  VR_CHECK_ARG(mos_shape_ok(S, B, ihm, iwm, H, W), "mosaic_seg_targets: bad shape (S %d, B %d, slots %d x %d, canvas %d x %d)", S, B,
               ihm, iwm, H, W);
  VR_CHECK_ARG(num_classes_seg > 0 && num_classes_seg < 255, "mosaic_seg_targets: 0 < num_classes_seg < 255, got %d",
               num_classes_seg);
  VR_CHECK_ARG(mos_st_lds_bytes(H, W) <= ST_LDS_MAX, "mosaic_seg_targets: a %d x %d canvas needs %ld bytes of LDS, above %ld", H, W,
               mos_st_lds_bytes(H, W), ST_LDS_MAX);
  VR_CHECK_ARG((long)B * H * W * (num_classes_seg + 1) < (1L << 40) && (long)ST_ROWS * W * (num_classes_seg + 1) < (1L << 31),
               "mosaic_seg_targets: batch too large");
  MosSegArgs p{};
  p.label = label; p.tab = mosaic;
  p.S = S; p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.ns = num_classes_seg;
  p.vec4 = ((long)W * (num_classes_seg + 1)) % 4 == 0 && vr_aligned16(onehot);
  p.png_out = png_out; p.onehot = onehot; p.flag = flag;
  hipLaunchKernelGGL(mosaic_seg_targets_kernel, dim3((unsigned)vr_cdiv(H, ST_ROWS), B), dim3(256), (size_t)mos_st_lds_bytes(H, W),
                     vr_stream(stream), p);
  VR_LAUNCH_CHECK("mosaic_seg_targets");
  return VR_OK;
}

extern "C" int vrnet_mosaic_box_targets_f32(const int* boxes, const int* counts, int S, const vrnet_mosaic_rec* mosaic, int B,
                                            int max_gt, int ihm, int iwm, int H, int W, float* targets, int* counts_out,
                                            int* flag, void* stream) {
  VR_CHECK_ARG(boxes && counts && mosaic && targets && counts_out,
               "mosaic_box_targets: boxes, counts, mosaic, targets and counts_out are required");
  VR_CHECK_ARG(mos_shape_ok(S, B, ihm, iwm, H, W) && max_gt > 0 && max_gt <= (1 << 20),
               "mosaic_box_targets: bad shape (S %d, B %d, max_gt %d, slots %d x %d, canvas %d x %d)", S, B, max_gt, ihm, iwm, H, W);
  MosBoxArgs p{};
  p.boxes = boxes; p.counts = counts; p.tab = mosaic;
  p.S = S; p.B = B; p.max_gt = max_gt; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W;
  p.targets = targets; p.counts_out = counts_out; p.flag = flag;
  hipLaunchKernelGGL(mosaic_box_targets_kernel, dim3(1, B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("mosaic_box_targets");
  return VR_OK;
}

extern "C" int vrnet_mosaic_radar_f32(const float* radar, int S, const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H,
                                      int W, float* out, int* flag, void* stream) {
  VR_CHECK_ARG(radar && mosaic && out && radar != out, "mosaic_radar: radar, mosaic and out are required, and out is not the input");
  VR_CHECK_ARG(mos_shape_ok(S, B, ihm, iwm, H, W) && (long)S * 4 * H * W < (1L << 40),
               "mosaic_radar: bad shape (S %d, B %d, slots %d x %d, canvas %d x %d)", S, B, ihm, iwm, H, W);
  MosRadarArgs p{};
  p.radar = radar; p.tab = mosaic;
  p.S = S; p.B = B; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W;
  p.out = out; p.flag = flag;
  hipLaunchKernelGGL(mosaic_radar_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, vr_stream(stream), p);
  VR_LAUNCH_CHECK("mosaic_radar");
  return VR_OK;
}

extern "C" long vrnet_mosaic_radar_points_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1L << 31)) return -1;
  return mos_points_bytes(B, H, W);
}

extern "C" int vrnet_mosaic_radar_points_f32(const float* points, int max_points, int S, const vrnet_radar_source* sources,
                                             const vrnet_mosaic_rec* mosaic, int B, int ihm, int iwm, int H, int W, int radius,
                                             float min_depth, float* out, int* flag, void* workspace, long workspace_bytes,
                                             void* stream) {
  VR_CHECK_ARG(points && sources && mosaic && out, "mosaic_radar_points: points, sources, mosaic and out are required");
  VR_CHECK_ARG(mos_shape_ok(S, B, ihm, iwm, H, W) && max_points > 0 && max_points <= (1 << 24) && (long)S * max_points < (1L << 31),
               "mosaic_radar_points: bad shape (S %d, max_points %d, B %d, slots %d x %d, canvas %d x %d)", S, max_points, B, ihm, iwm, H,
               W);
  VR_CHECK_ARG(radius >= 0 && radius <= 8, "mosaic_radar_points: 0 <= radius <= 8, got %d", radius);
  VR_CHECK_ARG(min_depth > 0.f && min_depth < INFINITY, "mosaic_radar_points: min_depth must be positive and finite, got %g",
               (double)min_depth);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(mosaic) & 7) == 0 && (reinterpret_cast<uintptr_t>(sources) & 7) == 0,
               "mosaic_radar_points: the record table and the source table must be 8-byte aligned");
  const long need = mos_points_bytes(B, H, W);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
    vr_set_error("mosaic_radar_points: workspace %ld < %ld bytes, or not 8-byte aligned", workspace ? workspace_bytes : 0L, need);
    return VR_ERR_WORKSPACE;
  }
  MosPointsArgs p{};
  p.points = points; p.src = sources; p.tab = mosaic;
  p.S = S; p.B = B; p.max_points = max_points; p.ihm = ihm; p.iwm = iwm; p.H = H; p.W = W; p.radius = radius;
  p.min_depth = min_depth;
  p.keys = static_cast<unsigned long long*>(workspace);
  p.out = out; p.flag = flag;
  hipStream_t st = vr_stream(stream);
  const long n = (long)B * H * W;
  hipLaunchKernelGGL(mosaic_radar_points_init_kernel, dim3((unsigned)vr_cdiv(n, 256)), dim3(256), 0, st, p.keys, n);
  hipLaunchKernelGGL(mosaic_radar_points_kernel, dim3((unsigned)vr_cdiv(max_points, 256), 4, B), dim3(256), 0, st, p);
  hipLaunchKernelGGL(mosaic_radar_points_resolve_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK("mosaic_radar_points");
  return VR_OK;
}
