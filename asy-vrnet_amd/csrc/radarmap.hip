// The radar input of the network from 4D radar POINTS, on the device: every point of an image is projected through the
// camera matrix of its view record into the window its frame went through (the letterbox window, or the window and flip of
// an augmentation record) and scattered into the (4, H, W) map, the nearest point winning a pixel.  The reference's data
// instructions ask for this map ("project 3D point clouds into 2D image plane, then make a numpy matrix with 4 x 512 x 512")
// and ship no code for it; the rule is this project's definition, stated on the host by data.radar_map, which these
// kernels equal bit for bit.  Against the integer gather of a finished map (augment.hip: radar) every point moves exactly
// once under an augmentation window: nothing is duplicated or dropped by resampling.
//
// Per point (x, y, z, f0..f3) of image b, in float32 with one rounding per operation (contraction off):
//   hu = ((P00 x + P01 y) + P02 z) + P03, hv and hw from rows 1 and 2; kept when hw >= min_depth and all three are finite
//   u = hu / hw, v = hv / hw; fx = (u * float(nw)) / float(iw), fy = (v * float(nh)) / float(ih); kept when 0 <= fx < nw, 0 <= fy < nh
//   ix = floor(fx), iy = floor(fy): window pixel (ix, iy) is canvas pixel (dx + ix, dy + iy) before the flip
//   it covers the canvas pixels within `radius` of that one (a square) that lie inside the canvas AND the window; with flip
//   the column is mirrored last (W - 1 - x), so the extent is the mirrored window's
// Per pixel the covering point with the smallest hw wins, the lowest index among equals: hw is positive and finite, so its
// bit pattern orders as an unsigned integer and key = bits(hw) << 32 | index orders the candidates; the winner is the minimum.
// Launches (grid y = image, the record loaded wave-uniformly):
//   init     one thread per pixel: key = ~0 (no candidate).  Every call starts from here, so no call sees an earlier one
//   points   one thread per point: project, then one 64-bit atomic minimum per covered pixel (at most (2 radius + 1)^2)
//   resolve  one thread per pixel: the key's low word names the winner; its four features go to the four planes as BITS
//            (NaN payloads survive), 0 where the key is still ~0; consecutive lanes store consecutive x
// Integer atomics only, and a minimum does not depend on the arrival order: the same bytes on every run.
//
// Under a rotation (vrnet_radar_map_post_f32: one vrnet_aug_post_rec per image beside the view record) the point pass moves
// the CENTRE of a kept point through the record's forward matrix -- data.radar_map(..., post=) is the rule -- so the "exactly
// once" above holds there too, where the nearest gather of a finished map (augment.hip: post radar) drops and duplicates
// isolated points.  In float64, every operation rounded on its own, left to right as the boxes take fwd:
//   rx = (fwd[0] X + fwd[1] Y) + fwd[2], ry = (fwd[3] X + fwd[4] Y) + fwd[5]; X' = floor(rx + 0.5), Y' = floor(ry + 0.5)
//   dropped when (X', Y') is outside the canvas; else the rectangle the point would cover without the rotation (cut to the
//   canvas and the window, mirrored under flip) is translated by (X' - X, Y' - Y) and cut to the canvas once more
// The square is not rotated and neither is the window's border.  The same three launches, key plane and resolve kernel; the
// point kernel is one body, the rotation a compile-time branch of it.
#include "postrec.h"
#include "radarpoint.h"

#pragma clang fp contract(off)

extern "C" {
/* include/vrnet_hip.h: the per-image view record of the radar map (80 bytes). */
typedef struct vrnet_radar_view {
  int ih, iw;                        /* the original frame the projection P is calibrated for */
  int nw, nh, dx, dy;                /* the window of the frame in the (H, W) canvas; may leave the canvas on every side */
  int flip, count;                   /* != 0: mirror the canvas left-right; points of this image */
  float P[12];                       /* (3, 4) row-major: (x, y, z, 1) -> homogeneous continuous pixel coordinates */
} vrnet_radar_view;
}
static_assert(sizeof(vrnet_radar_view) == 80 && alignof(vrnet_radar_view) == 4, "vrnet_radar_view layout");

namespace {

struct RadarMapArgs {
  const float* points;               // (B, max_points, 7)
  const vrnet_radar_view* views;     // (B)
  int B, max_points, H, W, radius;
  float min_depth;
  unsigned long long* keys;          // (B, H, W)
  float* out;                        // (B, 4, H, W)
  int* flag;                         // or null
  const vrnet_aug_post_rec* post;    // (B); the POST kernel only
  int max_angle;
};

__global__ __launch_bounds__(256) void radar_map_init_kernel(unsigned long long* keys, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = RM_EMPTY;
}

// POST: the image's post record is judged as the post kernels of augment.hip judge it, and a record that rotates moves the
// footprint of every kept point; !POST is the point pass of vrnet_radar_map_f32
template <bool POST>
__global__ __launch_bounds__(256) void radar_map_points_kernel(const RadarMapArgs p) {
  const int b = blockIdx.y;
  const vrnet_radar_view g = p.views[b];
  const bool bad = g.ih <= 0 || g.iw <= 0 || g.nw <= 0 || g.nh <= 0;
  const int count = vr_clampi(g.count, 0, p.max_points);
  bool qbad = false;
  PostRec q;
  if constexpr (POST) q = post_load(p.post, b, p.max_angle, qbad);
  if (blockIdx.x == 0 && threadIdx.x == 0 && p.flag) {
    const int bits = (bad || qbad ? VR_FLAG_GEOMETRY : 0) | (count != g.count ? VR_FLAG_POINT_COUNT : 0);
    if (bits) atomicOr(p.flag, bits);
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (bad || i >= count) return;
  const float* pt = p.points + ((long)b * p.max_points + i) * RM_POINT_FLOATS;
  int ix, iy;
  float hw;
  if (!rm_project(g.P, pt, p.min_depth, g.ih, g.iw, g.nw, g.nh, ix, iy, hw)) return;     // radarpoint.h
  // the centre in canvas coordinates before the flip; 64-bit: a hostile dx + ix must not wrap
  const long long cx = (long long)g.dx + ix, cy = (long long)g.dy + iy;
  // covered = the footprint cut by the canvas and by the window; every bound below is inside [0, W) x [0, H)
  const long long wx1 = (long long)g.dx + g.nw - 1, wy1 = (long long)g.dy + g.nh - 1;
  long long x0 = cx - p.radius, x1 = cx + p.radius, y0 = cy - p.radius, y1 = cy + p.radius;
  x0 = x0 < 0 ? 0 : x0;  x0 = x0 < g.dx ? g.dx : x0;
  y0 = y0 < 0 ? 0 : y0;  y0 = y0 < g.dy ? g.dy : y0;
  x1 = x1 > p.W - 1 ? p.W - 1 : x1;  x1 = x1 > wx1 ? wx1 : x1;
  y1 = y1 > p.H - 1 ? p.H - 1 : y1;  y1 = y1 > wy1 ? wy1 : y1;
  if (x0 > x1 || y0 > y1) return;
  if (g.flip) {                        // the columns of the finished canvas: still inside [0, W)
    const long long t = p.W - 1 - x1;
    x1 = p.W - 1 - x0;
    x0 = t;
  }
  if constexpr (POST) {
    if (q.rotate) {
      const long long X = g.flip ? p.W - 1 - cx : cx;          // |X| < 2^33: exact as a double
      const double rx = (q.fwd[0] * (double)X + q.fwd[1] * (double)cy) + q.fwd[2];
      const double ry = (q.fwd[3] * (double)X + q.fwd[4] * (double)cy) + q.fwd[5];
      const double fx = floor(rx + 0.5), fy = floor(ry + 0.5);
      if (!(fx >= 0.0 && fx < (double)p.W && fy >= 0.0 && fy < (double)p.H)) return;      // a NaN fails here too
      const long long tx = (int)fx - X, ty = (int)fy - cy;      // 0 <= fx < W, 0 <= fy < H
      x0 += tx;  x1 += tx;  y0 += ty;  y1 += ty;               // the cut rectangle follows its centre, then the canvas cuts it
      x0 = x0 < 0 ? 0 : x0;  x1 = x1 > p.W - 1 ? p.W - 1 : x1;
      y0 = y0 < 0 ? 0 : y0;  y1 = y1 > p.H - 1 ? p.H - 1 : y1;
      if (x0 > x1 || y0 > y1) return;
    }
  }
  const unsigned long long key = rm_key(hw, i);
  unsigned long long* plane = p.keys + (long)b * p.H * p.W;
  for (int yy = (int)y0; yy <= (int)y1; ++yy)
    for (int xx = (int)x0; xx <= (int)x1; ++xx) atomicMin(plane + (long)yy * p.W + xx, key);
}

__global__ __launch_bounds__(256) void radar_map_resolve_kernel(const RadarMapArgs p) {
  const long HW = (long)p.H * p.W;
  const long b = blockIdx.y, r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= HW) return;
  const unsigned long long key = p.keys[b * HW + r];
  const unsigned idx = (unsigned)key;
  unsigned f[4] = {0u, 0u, 0u, 0u};
  if (key != RM_EMPTY && idx < (unsigned)p.max_points) {       // the index of a key is below its image's count
    const unsigned* q = reinterpret_cast<const unsigned*>(p.points) + (b * p.max_points + idx) * RM_POINT_FLOATS + 3;
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = q[c];
  }
  unsigned* out = reinterpret_cast<unsigned*>(p.out);
#pragma unroll
  for (int c = 0; c < 4; ++c) out[(b * 4 + c) * HW + r] = f[c];
}

long radar_map_bytes(int B, int H, int W) { return (((long)B * H * W * 8) + 255) & ~255L; }

}  // namespace

extern "C" long vrnet_radar_map_workspace(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0 || (long)B * H * W >= (1L << 40)) return -1;
  return radar_map_bytes(B, H, W);
}

namespace {

// both entry points: post == nullptr is vrnet_radar_map_f32
int radar_map_run(const char* who, const float* points, int max_points, const vrnet_radar_view* views, int B, int H, int W,
                  int radius, float min_depth, const vrnet_aug_post_rec* post, int max_angle, float* out, int* flag,
                  void* workspace, long workspace_bytes, void* stream) {
  VR_CHECK_ARG(points && views && out, "%s: points, views and out are required", who);
  VR_CHECK_ARG(B > 0 && B < 65536 && max_points > 0 && max_points <= (1 << 24) && H > 0 && W > 0 && H < (1 << 24) &&
                   W < (1 << 24) && (long)B * 4 * H * W < (1L << 40),
               "%s: bad shape (B %d, max_points %d, canvas %d x %d)", who, B, max_points, H, W);
  VR_CHECK_ARG(radius >= 0 && radius <= 8, "%s: 0 <= radius <= 8, got %d", who, radius);
  VR_CHECK_ARG(min_depth > 0.f && min_depth < INFINITY, "%s: min_depth must be positive and finite, got %g", who,
               (double)min_depth);
  VR_CHECK_ARG((reinterpret_cast<uintptr_t>(views) & 7) == 0, "%s: the view table must be 8-byte aligned", who);
  VR_CHECK_ARG(!post || (reinterpret_cast<uintptr_t>(post) & 7) == 0, "%s: the post table must be 8-byte aligned", who);
  VR_CHECK_ARG(!post || (max_angle >= 0 && max_angle <= POST_MAX_ANGLE), "%s: 0 <= max_angle <= %d, got %d", who, POST_MAX_ANGLE,
               max_angle);
  const long need = radar_map_bytes(B, H, W);
  if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)) {
    vr_set_error("%s: workspace %ld < %ld bytes, or not 8-byte aligned", who, workspace ? workspace_bytes : 0L, need);
    return VR_ERR_WORKSPACE;
  }
  RadarMapArgs p{};
  p.points = points; p.views = views;
  p.B = B; p.max_points = max_points; p.H = H; p.W = W; p.radius = radius;
  p.min_depth = min_depth;
  p.keys = static_cast<unsigned long long*>(workspace);
  p.out = out; p.flag = flag;
  p.post = post; p.max_angle = max_angle;
  hipStream_t st = vr_stream(stream);
  const long n = (long)B * H * W;
  const dim3 pgrid((unsigned)vr_cdiv(max_points, 256), B);
  hipLaunchKernelGGL(radar_map_init_kernel, dim3((unsigned)vr_cdiv(n, 256)), dim3(256), 0, st, p.keys, n);
  if (post)
    hipLaunchKernelGGL(radar_map_points_kernel<true>, pgrid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL(radar_map_points_kernel<false>, pgrid, dim3(256), 0, st, p);
  hipLaunchKernelGGL(radar_map_resolve_kernel, dim3((unsigned)vr_cdiv((long)H * W, 256), B), dim3(256), 0, st, p);
  VR_LAUNCH_CHECK(who);
  return VR_OK;
}

}  // namespace

extern "C" int vrnet_radar_map_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, int H, int W,
                                   int radius, float min_depth, float* out, int* flag, void* workspace, long workspace_bytes,
                                   void* stream) {
  return radar_map_run("radar_map", points, max_points, views, B, H, W, radius, min_depth, nullptr, 0, out, flag, workspace,
                       workspace_bytes, stream);
}

extern "C" int vrnet_radar_map_post_f32(const float* points, int max_points, const vrnet_radar_view* views, int B, int H, int W,
                                        int radius, float min_depth, const vrnet_aug_post_rec* post, int max_angle, float* out,
                                        int* flag, void* workspace, long workspace_bytes, void* stream) {
  return radar_map_run(post ? "radar_map_post" : "radar_map", points, max_points, views, B, H, W, radius, min_depth, post, max_angle,
                       out, flag, workspace, workspace_bytes, stream);
}
