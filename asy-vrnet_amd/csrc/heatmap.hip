// Detection heat maps on the device: yolo.py:288-351 `detect_heatmap` (predict.py's `heatmap` mode) from the three raw
// detection maps (B, 5 + nc, h_l, w_l) at strides 8, 16 and 32 and the original frames, in three launches.
//   score     one thread per cell of the three levels: score = sigmoid(max_c cls_c) * sigmoid(obj) in fp32 (:339; the
//             sigmoid is monotone, so the max is taken on the logits), written to the workspace as planes (B, h_l, w_l),
//             an image's three levels back to back.  The first thread of image b also sets minmax[b] = (255, 0), so no
//             memset node precedes the atomics of the next launch.
//   mask      per output pixel and level the four bilinear taps of the score plane, blended horizontally then vertically
//             (cv2.resize INTER_LINEAR of the WHOLE level map, :340), times 255, truncated to a byte (:341), the max over
//             the levels (:342) -> mask (B, ih, iw) u8.  A workgroup is 64 x 4 threads on a tile 256 pixels wide and
//             `rows` high; a thread owns four horizontally adjacent pixels of rows / 4 consecutive rows, so its taps and
//             fractions along x are computed once per level and those along y once per row, and the horizontal blends
//             are kept from row to row while the two source rows stay the same.  One dword store per thread
//             and row where the four bytes lie on a 4-byte boundary, byte stores otherwise (rows of a width that is no
//             multiple of 4, the last group of a row).  The (min, max) of the image's own pixels: wave shuffles, LDS
//             atomics across the waves, then one integer atomicMin / atomicMax per workgroup -- order-free, so the pair
//             is the same on every run.
//   overlay   plt.imshow(mask, alpha, cmap="jet") (:344) at the frame's own resolution, not matplotlib's 200-dpi figure:
//             out = Image.blend(frame, jet[index(mask)], alpha) per byte (pixel.h).  matplotlib's default normalisation
//             takes vmin / vmax from the image, so each workgroup first builds its image's 256-entry colour table in
//             LDS: index(m) = trunc(((m - vmin) / (vmax - vmin)) * 256) in fp64, one rounding per operation, 256 -> 255,
//             and 0 for every m when vmax == vmin; `cmap` is the (256, 3) table.  Four pixels per thread: one dword of
//             mask and three of frame bytes in, three out (bytes when the tensors do not allow dwords).
// Taps.  window = 0 is the reference: linear_tap (pixel.h) with scale = w_l / iw, h_l / ih, whatever the letterbox did to
// the frame -- under a letterbox the grey bars are stretched over the picture with the rest.  window = 1 is this project's
// own aligned form: output pixel x is mapped through the letterbox window (dx, dy, nw, nh) of the W x H canvas into level
// coordinates, f = ((dx + ((x + 0.5) * nw) / iw) * w_l) / W - 0.5 in fp64, one rounding per operation, then the same
// floor and clamps (s < 0 -> (0, 0); s >= w_l - 1 -> (w_l - 1, 0)) with the fraction rounded to fp32; likewise in y.
// One body for both entry points (as segpost.hip): the size and window of image b are `geom` (vrnet_heatmap_f32: one
// record for every image, ihm, iwm = ih, iw) or tab[b] clamped by vr_geom_load (vrnet_heatmap_ragged_f32); mask and out
// are (B, ihm, iwm[, 3]) slots with image b in the top-left corner, 0 outside it, and the pair covers the image's own
// pixels only ((255, 0) for an image without pixels).  blockIdx.y is the image.  Every tap is clamped into its plane, so
// no record can move a read outside the workspace.
#include "common.h"
#include "pixel.h"

#pragma clang fp contract(off)

namespace {

struct HeatArgs {
  const float* lvl[3];               // (B, 5 + nc, h[l], w[l])
  int h[3], w[3];
  int soff[3];                       // floats from the start of an image's scores to its level l
  int sslot;                         // floats per image: the sum of h[l] * w[l]
  int B, nc, H, W, ihm, iwm;
  int window;
  int rows;                          // mask: rows per workgroup, a multiple of 4
  int vec;                           // overlay: the groups use dword accesses
  const vrnet_frame_geom* tab;       // RAGGED: (B) records
  vrnet_frame_geom geom;             // otherwise: the record of every image
  float* score;                      // (B, sslot)
  const unsigned char* frames;       // (B, ihm, iwm, 3)
  const unsigned char* cmap;         // (256, 3)
  float alpha;
  unsigned char* mask;               // (B, ihm, iwm)
  unsigned char* out;                // (B, ihm, iwm, 3)
  int* minmax;                       // (B, 2)
  int* flag;                         // or null
};

template <bool RAGGED>
__device__ __forceinline__ vrnet_frame_geom heat_geom(const HeatArgs& p, int b, bool& bad) {
  bad = false;
  if constexpr (RAGGED) return vr_geom_load(p.tab, b, p.ihm, p.iwm, p.H, p.W, bad);
  return p.geom;
}

__device__ __forceinline__ float heat_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void heat_score_kernel(const HeatArgs p) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) {
    p.minmax[2 * b] = 255;
    p.minmax[2 * b + 1] = 0;
  }
  if (e >= p.sslot) return;
  const int l = e >= p.soff[2] ? 2 : (e >= p.soff[1] ? 1 : 0);
  const float* base = l == 2 ? p.lvl[2] : (l == 1 ? p.lvl[1] : p.lvl[0]);
  const int off = l == 2 ? p.soff[2] : (l == 1 ? p.soff[1] : 0);
  const long plane = l == 2 ? (long)p.h[2] * p.w[2] : (l == 1 ? (long)p.h[1] * p.w[1] : (long)p.h[0] * p.w[0]);
  const float* src = base + (long)b * (5 + p.nc) * plane + (e - off);
  float m = src[5 * plane];
  for (int c = 1; c < p.nc; ++c) m = fmaxf(m, src[(5 + c) * plane]);
  p.score[(long)b * p.sslot + e] = heat_sigmoid(m) * heat_sigmoid(src[4 * plane]);
}

// the aligned form of one axis: output index d of `full` pixels, through the window [off, off + n) of a canvas of
// `canvas` pixels, into a level of `src` cells
__device__ __forceinline__ void window_tap(int d, int full, int off, int n, int src, int canvas, int& s0, int& s1, float& f) {
#pragma clang fp contract(off)
  const double t = (((double)d + 0.5) * (double)n) / (double)full;
  const double u = (double)off + t;
  const double c = (u * (double)src) / (double)canvas - 0.5;
  const double fl = floor(c);
  int s = (int)fl;
  f = (float)(c - fl);
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= src - 1) { s = src - 1; f = 0.f; }
  s0 = s;
  s1 = s + 1 < src ? s + 1 : s;
}

__device__ __forceinline__ void heat_tap(int window, int d, int full, int off, int n, int src, int canvas, int& s0, int& s1,
                                         float& f) {
  if (window) window_tap(d, full, off, n, src, canvas, s0, s1, f);
  else linear_tap(d, (float)src / (float)full, src, s0, s1, f);
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void heat_mask_kernel(const HeatArgs p) {
  __shared__ int s_mm[2];
  const int b = blockIdx.y, tx = threadIdx.x, ty = threadIdx.y;
  const bool lead = tx == 0 && ty == 0;
  bool bad;
  const vrnet_frame_geom g = heat_geom<RAGGED>(p, b, bad);
  if (bad && lead && blockIdx.x == 0 && p.flag) atomicOr(p.flag, VR_FLAG_GEOMETRY);
  if (lead) {
    s_mm[0] = 255;
    s_mm[1] = 0;
  }
  __syncthreads();
  const int ntx = (p.iwm + 255) / 256;
  const int strip = blockIdx.x / ntx, x0 = (blockIdx.x - strip * ntx) * 256 + 4 * tx;
  int xa[3][4], xb[3][4];
  float fx[3][4];
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xa[l][j] = xb[l][j] = 0;
      fx[l][j] = 0.f;
      if (x0 + j < g.iw) heat_tap(p.window, x0 + j, g.iw, g.dx, g.nw, p.w[l], p.W, xa[l][j], xb[l][j], fx[l][j]);
    }
  const float* sc = p.score + (long)b * p.sslot;
  const long slot = (long)p.ihm * p.iwm;
  // rows / 4 consecutive rows per thread: while the two source rows of a level stay the same, which they do for most
  // steps of an enlargement, the horizontal blends are kept and only the vertical one is redone -- the same values
  const int per = p.rows / 4, ybeg = strip * p.rows + ty * per, yend = min(ybeg + per, p.ihm);
  int py0[3] = {-1, -1, -1}, py1[3] = {-1, -1, -1};
  float top[3][4], bot[3][4];
  int mn = 255, mx = 0;
  for (int y = ybeg; y < yend; ++y) {
    unsigned int v4 = 0;                              // the padding of the slot
    if (y < g.ih && x0 < g.iw) {
      int best[4] = {0, 0, 0, 0};
#pragma unroll
      for (int l = 0; l < 3; ++l) {
        int y0, y1;
        float fy;
        heat_tap(p.window, y, g.ih, g.dy, g.nh, p.h[l], p.H, y0, y1, fy);
        if (y0 != py0[l] || y1 != py1[l]) {           // the same for the whole wave: a wave is one ty
          const float* r0 = sc + p.soff[l] + y0 * p.w[l];
          const float* r1 = sc + p.soff[l] + y1 * p.w[l];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float ax0 = 1.f - fx[l][j];
            top[l][j] = r0[xa[l][j]] * ax0 + r0[xb[l][j]] * fx[l][j];
            bot[l][j] = r1[xa[l][j]] * ax0 + r1[xb[l][j]] * fx[l][j];
          }
          py0[l] = y0;
          py1[l] = y1;
        }
        const float ay0 = 1.f - fy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = top[l][j] * ay0 + bot[l][j] * fy;
          best[j] = max(best[j], vr_clampi((int)(v * 255.f), 0, 255));
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < g.iw) {
          mn = min(mn, best[j]);
          mx = max(mx, best[j]);
          v4 |= (unsigned int)best[j] << (8 * j);
        }
    }
    if (x0 < p.iwm) {
      unsigned char* o = p.mask + b * slot + (long)y * p.iwm + x0;
      if (x0 + 4 <= p.iwm && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<unsigned int*>(o) = v4;
      } else {
        for (int j = 0; j < 4 && x0 + j < p.iwm; ++j) o[j] = (unsigned char)(v4 >> (8 * j));
      }
    }
  }
  // a wave is one ty: its 64 lanes all arrive here
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, 64));
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if (tx == 0 && mn <= mx) {
    atomicMin(&s_mm[0], mn);
    atomicMax(&s_mm[1], mx);
  }
  __syncthreads();
  if (lead && s_mm[0] <= s_mm[1]) {
    atomicMin(&p.minmax[2 * b], s_mm[0]);
    atomicMax(&p.minmax[2 * b + 1], s_mm[1]);
  }
}

template <bool RAGGED>
__global__ __launch_bounds__(256) void heat_overlay_kernel(const HeatArgs p) {
  __shared__ unsigned int s_lut[256];
  const int tid = threadIdx.x, b = blockIdx.y;
  bool bad;
  const vrnet_frame_geom g = heat_geom<RAGGED>(p, b, bad);
  {
    const int vmin = p.minmax[2 * b], vmax = p.minmax[2 * b + 1];
    int idx = 0;
    if (vmax > vmin) {
      const double t = ((double)(tid - vmin) / (double)(vmax - vmin)) * 256.0;
      idx = vr_clampi((int)t, 0, 255);               // 256 -> 255; values below vmin do not occur in the image
    }
    const unsigned char* c = p.cmap + 3 * idx;
    s_lut[tid] = (unsigned int)c[0] | ((unsigned int)c[1] << 8) | ((unsigned int)c[2] << 16);
  }
  __syncthreads();
  const int slot = p.ihm * p.iwm, ngroups = (slot + 3) / 4;
  const long base = (long)b * slot;
  for (int grp = blockIdx.x * 256 + tid; grp < ngroups; grp += gridDim.x * 256) {
    const int p0 = 4 * grp, npx = min(4, slot - p0);
    const bool dwords = p.vec && npx == 4;
    const unsigned char* m = p.mask + base + p0;
    const unsigned char* s = p.frames + 3L * (base + p0);
    unsigned int m4 = 0, f[3] = {0u, 0u, 0u};
    if (dwords) {
      m4 = *reinterpret_cast<const unsigned int*>(m);
      const unsigned int* s4 = reinterpret_cast<const unsigned int*>(s);
      f[0] = s4[0];
      f[1] = s4[1];
      f[2] = s4[2];
    } else {
      for (int j = 0; j < npx; ++j) m4 |= (unsigned int)m[j] << (8 * j);
      for (int j = 0; j < 3 * npx; ++j) f[j >> 2] |= (unsigned int)s[j] << (8 * (j & 3));
    }
    // the 12 bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3 as four packed pixels
    unsigned int px[4] = {f[0] & 0xFFFFFFu, (f[0] >> 24) | ((f[1] & 0xFFFFu) << 8), (f[1] >> 16) | ((f[2] & 0xFFu) << 16), f[2] >> 8};
    int y = p0 / p.iwm, x = p0 - y * p.iwm;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = !RAGGED || (y < g.ih && x < g.iw);
      const unsigned int c = s_lut[(m4 >> (8 * j)) & 255u], a = px[j];
      px[j] = !in ? 0u
                  : blend_byte(a & 255u, c & 255u, p.alpha) | (blend_byte((a >> 8) & 255u, (c >> 8) & 255u, p.alpha) << 8) |
                        (blend_byte((a >> 16) & 255u, (c >> 16) & 255u, p.alpha) << 16);
      if (++x == p.iwm) { x = 0; ++y; }
    }
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
}

bool heat_overlap(const void* a, long a_bytes, const void* b, long b_bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

long heat_score_floats(int H, int W) {
  return (long)(H / 8) * (W / 8) + (long)(H / 16) * (W / 16) + (long)(H / 32) * (W / 32);
}

// the argument checks that both entry points share; `ok`: the entry point's own conditions
int heat_check(const char* fn, bool ok, const float* p3, const float* p4, const float* p5, int B, int nc, int H, int W, int h,
               int w, const unsigned char* frames, const unsigned char* cmap, float alpha, const unsigned char* mask,
               const unsigned char* out, const int* minmax, const void* workspace, long workspace_bytes) {
  VR_CHECK_ARG(ok && p3 && p4 && p5 && mask && minmax && workspace && B > 0 && B < 65536 && nc >= 1 && H > 0 && W > 0 &&
                   H % 32 == 0 && W % 32 == 0 && (long)H * W < (1L << 31) && h > 0 && w > 0 && h <= (1 << 24) && w <= (1 << 24) &&
                   (long)h * w < (1L << 31) - 4,
               "%s: bad arguments (B %d, %d classes, input %d x %d: multiples of 32; output %d x %d, below 2^31 - 4 pixels)", fn, B, nc,
               H, W, h, w);
  VR_CHECK_ARG(alpha >= 0.f && alpha <= 1.f, "%s: alpha %g outside [0, 1]", fn, (double)alpha);
  VR_CHECK_ARG(!out || (frames && cmap), "%s: a picture (out) needs the frames and the colour table", fn);
  const long total = (long)B * h * w;
  VR_CHECK_ARG(!out || (!heat_overlap(out, 3 * total, frames, 3 * total) && !heat_overlap(out, 3 * total, mask, total)),
               "%s: out overlaps the frames or the mask", fn);
  const long need = (long)B * heat_score_floats(H, W) * (long)sizeof(float);
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3)) {
    vr_set_error("%s: workspace %ld < %ld bytes, or not 4-byte aligned", fn, workspace_bytes, need);
    return VR_ERR_WORKSPACE;
  }
  return VR_OK;
}

// the launches of both entry points; p carries everything but the derived fields
template <bool RAGGED>
void heat_launch(HeatArgs p, const float* p3, const float* p4, const float* p5, hipStream_t st) {
  p.lvl[0] = p3; p.lvl[1] = p4; p.lvl[2] = p5;
  int off = 0;
  for (int l = 0; l < 3; ++l) {
    p.h[l] = p.H / (8 << l);
    p.w[l] = p.W / (8 << l);
    p.soff[l] = off;
    off += p.h[l] * p.w[l];
  }
  p.sslot = off;
  hipLaunchKernelGGL(heat_score_kernel, dim3((unsigned)vr_cdiv(p.sslot, 256), p.B), dim3(256), 0, st, p);
  // rows per workgroup: 32, fewer while the launch would leave most of the chip without a workgroup
  const long ntx = vr_cdiv(p.iwm, 256);
  p.rows = 32;
  while (p.rows > 4 && (long)p.B * ntx * vr_cdiv(p.ihm, p.rows) < 512) p.rows /= 2;
  hipLaunchKernelGGL(heat_mask_kernel<RAGGED>, dim3((unsigned)(ntx * vr_cdiv(p.ihm, p.rows)), p.B), dim3(64, 4), 0, st, p);
  if (!p.out) return;
  // dword accesses: every slot starts on a 4-byte boundary in all three tensors
  const long slot = (long)p.ihm * p.iwm;
  p.vec = ((reinterpret_cast<uintptr_t>(p.frames) | reinterpret_cast<uintptr_t>(p.out) | reinterpret_cast<uintptr_t>(p.mask)) & 3) == 0 &&
          (slot % 4 == 0 || p.B == 1);
  long grid = vr_cdiv(vr_cdiv(slot, 4), 256);
  const long per_image = vr_cdiv(2048, p.B);
  if (grid > per_image) grid = per_image;
  hipLaunchKernelGGL(heat_overlay_kernel<RAGGED>, dim3((unsigned)grid, p.B), dim3(256), 0, st, p);
}

}  // namespace

extern "C" long vrnet_heatmap_workspace(int B, int H, int W) {
  return (long)B * heat_score_floats(H, W) * (long)sizeof(float);
}

extern "C" long vrnet_heatmap_ragged_workspace(int B, int H, int W) { return vrnet_heatmap_workspace(B, H, W); }

extern "C" int vrnet_heatmap_f32(const float* p3, const float* p4, const float* p5, int B, int nc, int H, int W, int ih, int iw,
                                 int window, int dx, int dy, int nw, int nh, const unsigned char* frames,
                                 const unsigned char* cmap, float alpha, unsigned char* mask, unsigned char* out, int* minmax,
                                 void* workspace, long workspace_bytes, void* stream) {
  if (const int rc = heat_check("heatmap", true, p3, p4, p5, B, nc, H, W, ih, iw, frames, cmap, alpha, mask, out, minmax,
                                workspace, workspace_bytes))
    return rc;
  VR_CHECK_ARG((window == 0 || window == 1) &&
                   (!window || (nw > 0 && nh > 0 && dx >= 0 && dy >= 0 && (long)dx + nw <= W && (long)dy + nh <= H)),
               "heatmap: window is 0 or 1, and the window dx %d dy %d %d x %d must lie inside %d x %d", dx, dy, nh, nw, H, W);
  HeatArgs p{};
  p.B = B; p.nc = nc; p.H = H; p.W = W; p.ihm = ih; p.iwm = iw; p.window = window;
  p.geom.ih = ih; p.geom.iw = iw;
  if (window) { p.geom.dx = dx; p.geom.dy = dy; p.geom.nw = nw; p.geom.nh = nh; }
  p.score = reinterpret_cast<float*>(workspace);
  p.frames = frames; p.cmap = cmap; p.alpha = alpha; p.mask = mask; p.out = out; p.minmax = minmax;
  heat_launch<false>(p, p3, p4, p5, vr_stream(stream));
  VR_LAUNCH_CHECK("heatmap");
  return VR_OK;
}

extern "C" int vrnet_heatmap_ragged_f32(const float* p3, const float* p4, const float* p5, const vrnet_frame_geom* geom, int B,
                                        int nc, int H, int W, int ihm, int iwm, int window, const unsigned char* frames,
                                        const unsigned char* cmap, float alpha, unsigned char* mask, unsigned char* out,
                                        int* minmax, int* flag, void* workspace, long workspace_bytes, void* stream) {
  if (const int rc = heat_check("heatmap_ragged", geom && (window == 0 || window == 1), p3, p4, p5, B, nc, H, W, ihm, iwm, frames,
                                cmap, alpha, mask, out, minmax, workspace, workspace_bytes))
    return rc;
  HeatArgs p{};
  p.tab = geom;
  p.B = B; p.nc = nc; p.H = H; p.W = W; p.ihm = ihm; p.iwm = iwm; p.window = window;
  p.score = reinterpret_cast<float*>(workspace);
  p.frames = frames; p.cmap = cmap; p.alpha = alpha; p.mask = mask; p.out = out; p.minmax = minmax; p.flag = flag;
  heat_launch<true>(p, p3, p4, p5, vr_stream(stream));
  VR_LAUNCH_CHECK("heatmap_ragged");
  return VR_OK;
}
